"""GPU: the native RCCL halo-exchange path on ONE rank.

Only 1-GPU boxes are available to the tests, so the communicator has a single rank and the domain is
made periodic: every face is sent to the rank itself (RCCL supports self send/recv inside a group).
That exercises exactly the code an 8-GPU run executes -- unique id, ncclCommInitRank, the plan's
pack kernels, ncclGroupStart/ncclSend/ncclRecv/ncclGroupEnd, unpack, the two-stream begin/end
choreography and the fused gt4mi_dist_lap5_f64 step -- against numpy's periodic wrap.
"""

import numpy as np
import pytest


def config_grid(line) -> str:
    return line["config"]["decomposition"]

pytestmark = pytest.mark.gpu


def _wrap(a, h, wrap_i=True, wrap_j=True):
    """Fill the ghost cells of a halo-padded array periodically (two-phase, corners included)."""
    a = a.copy()
    if wrap_i:
        a[:h] = a[-2 * h:-h]
        a[-h:] = a[h:2 * h]
    if wrap_j:
        a[:, :h] = a[:, -2 * h:-h]
        a[:, -h:] = a[:, h:2 * h]
    return a


@pytest.fixture(scope="module")
def comm():
    from gt4py_amd.distributed import NativeComm

    c = NativeComm(rank=0, world_size=1)
    yield c
    c.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("periodic", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("halo", [1, 2])
def test_periodic_self_exchange(comm, dtype, periodic, halo):
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger

    gd = (37, 22, 5)
    dec = Decomposition(gd, (1, 1), 0, halo, periodic=periodic)
    rng = np.random.default_rng(3)
    host = rng.uniform(-1, 1, dec.local_shape).astype(dtype)
    dev = gt_storage.from_array(host, dtype, backend="hip:mi300", aligned_index=dec.origin)
    ex = NativeHaloExchanger(dec, dtype, comm)
    ex.exchange(dev)
    torch.cuda.synchronize()
    assert np.array_equal(dev.get(), _wrap(host, halo, *periodic))
    assert ex.bytes_per_exchange > 0
    # overlapped form gives the same result
    dev2 = gt_storage.from_array(host, dtype, backend="hip:mi300", aligned_index=dec.origin)
    ex.begin(dev2)
    ex.end()
    torch.cuda.synchronize()
    assert np.array_equal(dev2.get(), _wrap(host, halo, *periodic))
    ex.close()


@pytest.mark.parametrize("edge_columns,schedule", [(None, None), (1, "join"), (8, "chain"), (16, "chain"), (6, "join"), (8, "swap"),
                                                   (16, "swap"), (1, "swap"), (8, "swap-packed"), (16, "swap-packed")])
@pytest.mark.parametrize("periodic", [(True, True), (False, True), (True, False)])
def test_fused_distributed_laplacian_step(comm, periodic, edge_columns, schedule):
    """gt4mi_dist_lap5_f64 (exchange || interior, then the ring) == oracle Laplacian on the wrapped field, for every width
    of the W / E boxes the ring takes off the interior and both schedules."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from oracle import ref_numpy as R

    gd = (64, 48, 6) if edge_columns != 16 else (300, 40, 4)  # 16 columns need a local domain at least 256 wide
    dec = Decomposition(gd, (1, 1), 0, 1, periodic=periodic)
    rng = np.random.default_rng(11)
    host = rng.uniform(-1, 1, dec.local_shape)
    inp = gt_storage.from_array(host, backend="hip:mi300", aligned_index=(1, 1, 0))
    out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=(1, 1, 0))
    ex = NativeHaloExchanger(dec, np.float64, comm)
    if edge_columns is not None:
        ex.tune(schedule, 0, edge_columns=edge_columns)
    step = ex.make_dist_lap5(inp, out, (1, 1, 0), (1, 1, 0))
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    wrapped = _wrap(host, 1, *periodic)
    want = np.zeros_like(host)
    R.laplacian(wrapped, want)
    assert np.array_equal(out.get(), want)
    assert np.array_equal(inp.get(), wrapped)
    ex.close()


@pytest.mark.parametrize("literal32", [False, True])
@pytest.mark.parametrize("schedule", ["join", "chain", "swap", "swap-packed"])
def test_fused_distributed_laplacian_step_float32(comm, schedule, literal32):
    """gt4mi_dist_lap5_f32: the same step on float32 fields (a plan of 4-byte items), both literal precisions -- equal to the
    whole-domain kernel on the exchanged field, and for float32 literals to the oracle's all-float32 Laplacian."""
    import ctypes

    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from gt4py_amd.distributed.native import _field_struct
    from oracle import ref_numpy as R

    flags = _lib.LAP_LITERAL_F32 if literal32 else 0
    dec = Decomposition((300, 40, 4), (1, 1), 0, 1, periodic=(True, True))
    host = np.random.default_rng(13).uniform(-1, 1, dec.local_shape).astype(np.float32)
    inp = gt_storage.from_array(host, np.float32, backend="hip:mi300", aligned_index=dec.origin)
    out = gt_storage.zeros(dec.local_shape, np.float32, backend="hip:mi300", aligned_index=dec.origin)
    ref = gt_storage.zeros(dec.local_shape, np.float32, backend="hip:mi300", aligned_index=dec.origin)
    ex = NativeHaloExchanger(dec, np.float32, comm).tune(schedule, 0)
    step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin, flags=flags)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    wrapped = _wrap(host, 1, True, True)
    assert np.array_equal(inp.get(), wrapped)
    lib = _lib.load()
    fi, fo = _field_struct(inp, dec.origin), _field_struct(ref, dec.origin)
    _lib.check("gt4mi_lap5_f32", lib.gt4mi_lap5_f32(_lib.domain3(dec.local_domain), ctypes.byref(fi), ctypes.byref(fo), 0, flags,
                                                    torch.cuda.current_stream().cuda_stream, None))
    torch.cuda.synchronize()
    assert np.array_equal(out.get(), ref.get())
    if literal32:
        want = np.zeros_like(host)
        R.laplacian(wrapped, want)
        assert np.array_equal(out.get(), want)
    # ... and on the direct transport, cut along J only: push, interior and the edge units in ONE launch (lap5_edge.hip.h), both
    # message tables, a width that is no multiple of the tile and fewer levels than a wave takes
    if schedule == "join":
        for gd in ((300, 40, 5), (1024, 6, 19)):
            dj = Decomposition(gd, (1, 1), 0, 1, periodic=(False, True))
            hostj = np.random.default_rng(17).uniform(-1, 1, dj.local_shape).astype(np.float32)
            for single_phase in (False, True):
                a = gt_storage.from_array(hostj, np.float32, backend="hip:mi300", aligned_index=dj.origin)
                b = gt_storage.zeros(dj.local_shape, np.float32, backend="hip:mi300", aligned_index=dj.origin)
                r = gt_storage.zeros(dj.local_shape, np.float32, backend="hip:mi300", aligned_index=dj.origin)
                exd = _direct(NativeHaloExchanger(dj, np.float32, comm, single_phase=single_phase).tune("inline", 0))
                fused = exd.make_dist_lap5(a, b, dj.origin, dj.origin, flags=flags)
                for _ in range(3):
                    fused()
                torch.cuda.synchronize()
                wrapped_j = _wrap(hostj, 1, False, True)
                assert np.array_equal(a.get(), wrapped_j), (gd, single_phase)
                fa, fr = _field_struct(a, dj.origin), _field_struct(r, dj.origin)
                _lib.check("gt4mi_lap5_f32", lib.gt4mi_lap5_f32(_lib.domain3(dj.local_domain), ctypes.byref(fa), ctypes.byref(fr), 0, flags,
                                                                torch.cuda.current_stream().cuda_stream, None))
                torch.cuda.synchronize()
                assert np.array_equal(b.get(), r.get()), (gd, single_phase)
                assert exd.direct_status()["timed_out"] is False
                exd.close()
    # a plan of 8-byte items refuses float32 fields instead of moving half of every face
    ex8 = NativeHaloExchanger(dec, np.float64, comm)
    ex8.itemsize = 4  # (get past the Python-side choice of the entry point)
    with pytest.raises(RuntimeError, match="8-byte items"):
        ex8.make_dist_lap5(inp, out, dec.origin, dec.origin)()
    ex8.close()
    ex.close()


def test_overlapped_apply_with_native_exchanger(comm):
    """The generic Python driver (any stencil family) on top of the native exchanger: hdiff, halo 2."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger, overlapped_apply
    from oracle import ref_numpy as R

    hd = gtscript.stencil(backend="hip:mi300", definition=hip_templates.hdiff_limiter_field,
                          dtypes={"T": np.float64}, device_sync=False)
    gd = (40, 36, 3)
    dec = Decomposition(gd, (1, 1), 0, 2, periodic=(True, True))
    rng = np.random.default_rng(5)
    host = rng.uniform(-10, 10, dec.local_shape)
    coeff = rng.uniform(0, 0.5, dec.local_shape)
    d_in = gt_storage.from_array(host, backend="hip:mi300", aligned_index=dec.origin)
    d_cf = gt_storage.from_array(coeff, backend="hip:mi300", aligned_index=dec.origin)
    d_out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
    ex = NativeHaloExchanger(dec, np.float64, comm)
    origin = {n: dec.origin for n in ("in_field", "out_field", "coeff")}
    overlapped_apply(hd, dec, origin, {"in_field": d_in, "out_field": d_out, "coeff": d_cf}, {"in_field": ex})
    torch.cuda.synchronize()
    want = np.zeros_like(host)
    R.hdiff(_wrap(host, 2), want, coeff, domain=gd)
    assert np.array_equal(d_out.get(), want)
    # the stencil-agnostic schedule (fork, begin, interior, end, strips -- no fused step) on either transport
    for direct in (False, True):
        if direct:
            _direct(ex)
        for _ in range(2):
            fresh = gt_storage.from_array(host, backend="hip:mi300", aligned_index=dec.origin)
            d_out.tensor.zero_()
            overlapped_apply(hd, dec, origin, {"in_field": fresh, "out_field": d_out, "coeff": d_cf}, {"in_field": ex}, fused=False)
            torch.cuda.synchronize()
            assert np.array_equal(d_out.get(), want), direct
            assert np.array_equal(fresh.get(), _wrap(host, 2)), direct
    ex.close()


@pytest.mark.parametrize("periodic", [(False, True), (True, True), (True, False)])
def test_pipelined_time_stepping(comm, periodic):
    """gt4mi_dist_lap5_f64_pipelined: n steps of u <- lap(u) on a periodic domain (ghost cells of the
    freshly written field exchanged next to the interior kernel) == n oracle steps with numpy wrap."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from oracle import ref_numpy as R

    gd = (64, 40, 5)
    dec = Decomposition(gd, (1, 1), 0, 1, periodic=periodic)
    rng = np.random.default_rng(21)
    host = rng.uniform(-1, 1, dec.local_shape) * 1e-3
    a = gt_storage.from_array(host, backend="hip:mi300", aligned_index=(1, 1, 0))
    b = gt_storage.from_array(host * 0 + 7.0, backend="hip:mi300", aligned_index=(1, 1, 0))
    ex = NativeHaloExchanger(dec, np.float64, comm)
    step = ex.make_time_stepper_lap5(a, b, (1, 1, 0))
    nsteps = 7
    for _ in range(nsteps):
        step()
    ex.end()
    torch.cuda.synchronize()
    # oracle: non-periodic ghost cells of the OUTPUT buffers keep whatever they held (host / 7.0)
    u, v = host.copy(), host * 0 + 7.0
    for _ in range(nsteps):
        u = _wrap(u, 1, *periodic)
        R.laplacian(u, v)
        u, v = v, u
    u = _wrap(u, 1, *periodic)
    got = step.result().get()
    assert np.array_equal(got, u)
    ex.close()
    with pytest.raises(Exception, match="never exchanged"):
        ex2 = NativeHaloExchanger(dec, np.float64, comm)
        f = __import__("gt4py_amd.distributed.native", fromlist=["_field_struct"])._field_struct
        import ctypes

        from gt4py_amd import _lib

        fa, fb = f(a, (1, 1, 0)), f(b, (1, 1, 0))
        _lib.check("x", ex2._lib.gt4mi_dist_lap5_f64_pipelined(ex2._plan, _lib.domain3(gd), ctypes.byref(fa), ctypes.byref(fb),
                                                               0, ex2.sides, None))


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("nsteps", [1, 4, 7])
@pytest.mark.parametrize("halo", [1, 2, 3, 4])
@pytest.mark.parametrize("periodic", [(False, True), (True, True)])
def test_wide_halo_time_stepping(comm, periodic, halo, nsteps, overlap, direct):
    """gt4mi_dist_lap5_f64_wide: ghost regions `halo` deep, one exchange per `halo` steps, redundant
    rows computed in between; the compute domain after n steps equals n oracle steps with a fresh
    periodic wrap every step."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from oracle import ref_numpy as R

    gd = (48, 40, 4)
    dec = Decomposition(gd, (1, 1), 0, halo, periodic=periodic)
    o = dec.origin
    rng = np.random.default_rng(100 + halo)
    host = rng.uniform(-1, 1, dec.local_shape) * 1e-3
    a = gt_storage.from_array(host, backend="hip:mi300", aligned_index=o)
    b = gt_storage.from_array(host * 0 + 7.0, backend="hip:mi300", aligned_index=o)
    ex = NativeHaloExchanger(dec, np.float64, comm)
    if direct:  # the faces pushed by the pack kernel instead of RCCL send/recv
        _direct(ex)
    step = ex.make_time_stepper_lap5(a, b, o, overlap=overlap)
    for _ in range(nsteps):
        step()
    torch.cuda.synchronize()
    # oracle on a depth-1 halo view: only the compute domain is compared
    h = halo
    core = (slice(h - 1, -(h - 1)) if h > 1 else slice(None),) * 2 + (slice(None),)
    u, v = host[core].copy(), (host * 0 + 7.0)[core].copy()
    for _ in range(nsteps):
        u = _wrap(u, 1, *periodic)
        R.laplacian(u, v)
        u, v = v, u
    got = step.result().get()[core]
    assert np.array_equal(got[1:-1, 1:-1], u[1:-1, 1:-1])
    ex.close()


def test_sequential_and_tuned_apply_match_the_overlapped_form(comm):
    """sequential_apply (exchange, then one full-domain launch) and TunedApply (measures, keeps the faster) on
    the generic driver: same values as the oracle on the periodic self-loop, hdiff with ghost depth 2."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger, TunedApply, sequential_apply
    from oracle import ref_numpy as R

    hd = gtscript.stencil(backend="hip:mi300", definition=hip_templates.hdiff_limiter_field,
                          dtypes={"T": np.float64}, device_sync=False)
    gd = (40, 36, 3)
    dec = Decomposition(gd, (1, 1), 0, 2, periodic=(True, True))
    rng = np.random.default_rng(6)
    host = rng.uniform(-10, 10, dec.local_shape)
    coeff = rng.uniform(0, 0.5, dec.local_shape)
    want = np.zeros_like(host)
    R.hdiff(_wrap(host, 2), want, coeff, domain=gd)
    origin = {n: dec.origin for n in ("in_field", "out_field", "coeff")}
    for form in ("sequential", "tuned"):
        d_in = gt_storage.from_array(host, backend="hip:mi300", aligned_index=dec.origin)
        d_cf = gt_storage.from_array(coeff, backend="hip:mi300", aligned_index=dec.origin)
        d_out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
        ex = NativeHaloExchanger(dec, np.float64, comm)
        args = {"in_field": d_in, "out_field": d_out, "coeff": d_cf}
        if form == "sequential":
            sequential_apply(hd, dec, origin, args, {"in_field": ex})
        else:
            tuned = TunedApply(hd, dec, origin, {"in_field": ex})
            tuned(args)
            assert tuned.choice in ("overlapped", "sequential") and set(tuned.timings_ms) == {"overlapped", "sequential"}
            tuned(args)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.get(), want), form
        ex.close()


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("side", ["N", "S"])
@pytest.mark.parametrize("halo", [1, 2, 3])
def test_one_sided_rank(comm, halo, side, overlap):
    """A rank with a neighbour on ONE J side only (what ranks 0 and N-1 of a bounded 1xN grid are): the plan
    delivers that side's ghost rows (here from the rank's own opposite rows, the only peer a 1-GPU box has),
    the other side is a physical boundary whose ghost rows never change.  Checked against the same scheme
    written in numpy with the oracle's Laplacian."""
    import ctypes

    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from oracle import ref_numpy as R

    H = halo
    gd = (40, 24, 3)
    dec = Decomposition(gd, (1, 1), 0, H, periodic=(False, True))
    ex = NativeHaloExchanger(dec, np.float64, comm)
    # replace the two-sided periodic plan by a one-sided one
    ex.close()
    li, lj, lk = gd
    # a rank sends the face that lies on its neighbour's side (the overlapped step computes exactly those rows
    # before packing); with itself as the only available peer, that face comes back as its own ghost rows
    if side == "N":  # my last H rows -> my N ghost rows
        send = _lib.HaloMsg.make(0, 1, (0, lj, 0), (li + 2 * H, H, lk))
        recv = _lib.HaloMsg.make(0, 1, (0, H + lj, 0), (li + 2 * H, H, lk))
        sides = 8
    else:  # my first H rows -> my S ghost rows
        send = _lib.HaloMsg.make(0, 1, (0, H, 0), (li + 2 * H, H, lk))
        recv = _lib.HaloMsg.make(0, 1, (0, 0, 0), (li + 2 * H, H, lk))
        sides = 4
    plan = ctypes.c_void_p()
    lib = _lib.load()
    _lib.check("gt4mi_halo_plan_create", lib.gt4mi_halo_plan_create(comm.handle, 8, (_lib.HaloMsg * 1)(send), 1,
                                                                   (_lib.HaloMsg * 1)(recv), 1, ctypes.byref(plan)))
    ex._plan, ex.sides = plan, sides

    rng = np.random.default_rng(17 + H)
    host = rng.uniform(-1, 1, dec.local_shape) * 1e-3
    o = dec.origin

    def deliver(f):  # what the plan does to a host array
        if side == "N":
            f[:, H + lj:H + lj + H] = f[:, lj:lj + H]
        else:
            f[:, 0:H] = f[:, H:2 * H]

    deliver(host)
    a = gt_storage.from_array(host, backend="hip:mi300", aligned_index=o)
    b = gt_storage.from_array(host.copy(), backend="hip:mi300", aligned_index=o)
    step = ex.make_time_stepper_lap5(a, b, o, overlap=overlap)
    nsteps = 2 * H + 1
    for _ in range(nsteps):
        step()
    torch.cuda.synchronize()

    u, v = host.copy(), host.copy()
    for n in range(nsteps):
        ext = H - 1 - n % H
        lo_j = H - (ext if side == "S" else 0)
        hi_j = H + lj + (ext if side == "N" else 0)
        view = (slice(H - 1, H + li + 1), slice(lo_j - 1, hi_j + 1), slice(None))
        R.laplacian(u[view], v[view])
        if ext == 0:
            deliver(v)
        u, v = v, u
    got = step.result().get()
    assert np.array_equal(got[H:H + li, H:H + lj], u[H:H + li, H:H + lj])
    ex.close()


@pytest.mark.parametrize("form", ["overlapped", "sequential"])
def test_baseline_config4_share_with_all_four_neighbours(comm, form):
    """BASELINE.json configs[4] at the size ONE rank of the 4 x 2 grid holds: fp64 horizontal diffusion on
    512 x 1024 x 80 with ghost depth 2.  The domain is periodic along both axes, so W, E, S and N (and, through the
    two-phase exchange, the four corners) are all live -- each is the rank itself over RCCL.  Slabs of the result
    are compared with the oracle on the periodically wrapped field: horizontal diffusion is PARALLEL in K, so a
    few levels of the full 512 x 1024 plane -- including every boundary strip and corner -- check the kernels,
    the strips and the exchange without a multi-gigabyte numpy evaluation."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger, overlapped_apply, sequential_apply
    from oracle import ref_numpy as R

    hd = gtscript.stencil(backend="hip:mi300", definition=hip_templates.hdiff_limiter_field,
                          dtypes={"T": np.float64}, device_sync=False)
    gd, h = (512, 1024, 80), 2
    dec = Decomposition(gd, (1, 1), 0, h, periodic=(True, True))
    assert dec.local_shape == (516, 1028, 80) and all(v == 0 for v in dec.neighbours.values())
    gen = torch.Generator(device="cuda").manual_seed(20262)
    fields = {}
    for name, lo, hi in (("in_field", -10.0, 10.0), ("coeff", 0.0, 0.5), ("out_field", 0.0, 0.0)):
        f = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
        if hi > lo:
            f.tensor.copy_(torch.rand(dec.local_shape, dtype=torch.float64, device="cuda", generator=gen) * (hi - lo) + lo)
        fields[name] = f
    levels = [0, 1, 39, 78, 79]
    host_in = fields["in_field"].tensor[:, :, levels].cpu().numpy()  # ghost cells still hold their random values
    host_cf = fields["coeff"].tensor[:, :, levels].cpu().numpy()
    ex = NativeHaloExchanger(dec, np.float64, comm)
    assert ex.bytes_per_exchange == 2 * (2 * 1024 * 80 * 8) + 2 * (516 * 2 * 80 * 8)  # 3.94 MB: 2 I faces + 2 J faces (with the fresh I-halo columns)
    origin = {n: dec.origin for n in fields}
    apply = overlapped_apply if form == "overlapped" else sequential_apply
    apply(hd, dec, origin, fields, {"in_field": ex})
    torch.cuda.synchronize()
    want = np.zeros_like(host_in)
    wrapped = _wrap(host_in, h)
    R.hdiff(wrapped, want, host_cf, domain=(gd[0], gd[1], len(levels)))
    got = fields["out_field"].tensor[:, :, levels].cpu().numpy()
    assert np.array_equal(got[h:-h, h:-h], want[h:-h, h:-h])
    # the exchange refreshed the input's ghost cells with the periodic images, corners included
    assert np.array_equal(fields["in_field"].tensor[:, :, levels].cpu().numpy(), wrapped)
    # size-independent property on ALL 80 levels: a field that is linear in i and j has lap == 0, hence out == in
    # exactly; with the periodic wrap that holds away from the seam
    ii = torch.arange(dec.local_shape[0], dtype=torch.float64, device="cuda")[:, None, None]
    jj = torch.arange(dec.local_shape[1], dtype=torch.float64, device="cuda")[None, :, None]
    fields["in_field"].tensor.copy_((3.0 * ii + 5.0 * jj + 7.0).expand(dec.local_shape))
    apply(hd, dec, origin, fields, {"in_field": ex})
    torch.cuda.synchronize()
    out, inp = fields["out_field"].tensor, fields["in_field"].tensor
    inner = (slice(h + 2, -(h + 2)), slice(h + 2, -(h + 2)), slice(None))
    assert torch.equal(out[inner], inp[inner])
    ex.close()


# ---- round 3: fused distributed horizontal diffusion, single-phase plans, the time-skewed stepper ---------------------
def test_communicator_reports_what_rccl_sees(comm):
    info = comm.info()
    assert info["nranks"] == 1 and info["rank"] == 0 and info["device"] >= 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("periodic", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("halo", [1, 2])
def test_single_phase_self_exchange(comm, dtype, periodic, halo):
    """The 8-neighbour table (faces + corner boxes in ONE round) refreshes exactly the cells the two-phase table does."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger

    dec = Decomposition((37, 22, 5), (1, 1), 0, halo, periodic=periodic)
    rng = np.random.default_rng(3)
    host = rng.uniform(-1, 1, dec.local_shape).astype(dtype)
    dev = gt_storage.from_array(host, dtype, backend="hip:mi300", aligned_index=dec.origin)
    ex = NativeHaloExchanger(dec, dtype, comm, single_phase=True)
    ex.exchange(dev)
    torch.cuda.synchronize()
    assert np.array_equal(dev.get(), _wrap(host, halo, *periodic))
    ex.close()


@pytest.mark.parametrize("single_phase", [False, True])
@pytest.mark.parametrize("periodic", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("dtype,coeff_kind", [(np.float64, "field"), (np.float32, "field"), (np.float64, "scalar")])
@pytest.mark.parametrize("gd", [(40, 36, 3), (130, 70, 4)])
def test_fused_distributed_hdiff_step(comm, gd, dtype, coeff_kind, periodic, single_phase):
    """gt4mi_dist_hdiff_*: pack, interior next to the exchange, ONE ring kernel == oracle on the wrapped field; reached
    through the stencil-agnostic driver (overlapped_apply picks the fused step for a kernel-library stencil)."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger, fused_apply, overlapped_apply
    from oracle import ref_numpy as R

    defn = hip_templates.hdiff_limiter_field if coeff_kind == "field" else hip_templates.hdiff_limiter_scalar
    dtypes = {"T": dtype} if coeff_kind == "field" else {"T": dtype, "S": np.float64}
    hd = gtscript.stencil(backend="hip:mi300", definition=defn, dtypes=dtypes, device_sync=False)
    dec = Decomposition(gd, (1, 1), 0, 2, periodic=periodic)
    rng = np.random.default_rng(5)
    host = rng.uniform(-10, 10, dec.local_shape).astype(dtype)
    coeff = rng.uniform(0, 0.5, dec.local_shape).astype(dtype)
    d_in = gt_storage.from_array(host, dtype, backend="hip:mi300", aligned_index=dec.origin)
    d_out = gt_storage.zeros(dec.local_shape, dtype, backend="hip:mi300", aligned_index=dec.origin)
    ex = NativeHaloExchanger(dec, dtype, comm, single_phase=single_phase)
    if gd[0] > 100:  # the wide domain: other widths of the W / E boxes than the default, and every schedule
        case = (1 if single_phase else 0) + 2 * (0 if all(periodic) else (1 if periodic[1] else 2))
        ex.tune(("join", "chain", "swap", "swap-packed")[case % 4], 3, edge_columns=8 if periodic[1] else 32)
    names = list(inspect_signature_names(hd))
    args = {names[0]: d_in, names[1]: d_out}
    if coeff_kind == "field":
        args[names[2]] = gt_storage.from_array(coeff, dtype, backend="hip:mi300", aligned_index=dec.origin)
        oracle_coeff = coeff
    else:
        args[names[2]] = 0.21
        oracle_coeff = np.float64(0.21)
    origin = {n: dec.origin for n in names[:3] if not isinstance(args[n], float)}
    assert fused_apply(hd, dec, origin, args, {names[0]: ex})  # the combination IS covered by the native step
    d_out.tensor.zero_()
    for _ in range(2):
        overlapped_apply(hd, dec, origin, args, {names[0]: ex})
    torch.cuda.synchronize()
    wrapped = _wrap(host, 2, *periodic)
    want = np.zeros_like(host)
    R.hdiff(wrapped, want, oracle_coeff, domain=gd)
    assert np.array_equal(d_out.get(), want)
    assert np.array_equal(d_in.get(), wrapped)
    ex.close()


def inspect_signature_names(stencil):
    import inspect

    return inspect.signature(stencil.definition_func).parameters


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("single_phase", [False, True])
@pytest.mark.parametrize("halo", [1, 2, 3])
@pytest.mark.parametrize("periodic", [(False, True), (True, True), (True, False)])
@pytest.mark.parametrize("gd", [(48, 40, 4), (130, 36, 3)])
def test_time_skewed_stepping(comm, gd, periodic, halo, single_phase, direct):
    """gt4mi_dist_lap5_f64_skewed: per cycle the bands of steps 1 .. H, then the exchange next to the H interior kernels;
    after n cycles the compute domain equals n * H oracle steps with a fresh periodic wrap every step."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from oracle import ref_numpy as R

    dec = Decomposition(gd, (1, 1), 0, halo, periodic=periodic)
    o = dec.origin
    rng = np.random.default_rng(200 + halo)
    host = rng.uniform(-1, 1, dec.local_shape) * 1e-3
    a = gt_storage.from_array(host, backend="hip:mi300", aligned_index=o)
    # Both buffers carry the fixed physical-boundary ring -- also where it crosses the ghost rows of a neighbour: from a ghost
    # depth of 3 on, the grown bands read those cells of the buffer that is NOT exchanged in that cycle (a decomposed run has
    # them from the initial scatter of the global array; on the periodic self-loop they are the wrapped images).
    b = gt_storage.from_array(_wrap(host, halo, *periodic), backend="hip:mi300", aligned_index=o)
    ex = NativeHaloExchanger(dec, np.float64, comm, single_phase=single_phase)
    if direct:
        _direct(ex)
    cycle = ex.make_time_skewed_lap5(a, b, o)
    assert cycle.steps_per_call == halo
    ncycles = 3
    for _ in range(ncycles):
        cycle()
    ex.end()
    torch.cuda.synchronize()
    h = halo
    core = (slice(h - 1, -(h - 1)) if h > 1 else slice(None),) * 2 + (slice(None),)
    u, v = host[core].copy(), host[core].copy()
    for _ in range(ncycles * halo):
        u = _wrap(u, 1, *periodic)
        R.laplacian(u, v)
        u, v = v, u
    got = cycle.result().get()[core]
    assert np.array_equal(got[1:-1, 1:-1], u[1:-1, 1:-1])
    ex.close()


@pytest.mark.parametrize("single_phase", [False, True])
def test_baseline_config4_share_through_the_fused_native_step(comm, single_phase):
    """BASELINE.json configs[4]'s per-rank share (512 x 1024 x 80 fp64, ghost depth 2, all four neighbours and the corners
    live on the periodic self-loop) through gt4mi_dist_hdiff_f64: slabs against the oracle, ghost cells refreshed, and the
    size-independent linear-field property on all 80 levels -- the same checks as the driver-level test above."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger, fused_apply
    from oracle import ref_numpy as R

    hd = gtscript.stencil(backend="hip:mi300", definition=hip_templates.hdiff_limiter_field,
                          dtypes={"T": np.float64}, device_sync=False)
    gd, h = (512, 1024, 80), 2
    dec = Decomposition(gd, (1, 1), 0, h, periodic=(True, True))
    gen = torch.Generator(device="cuda").manual_seed(20263)
    fields = {}
    for name, lo, hi in (("in_field", -10.0, 10.0), ("coeff", 0.0, 0.5), ("out_field", 0.0, 0.0)):
        f = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
        if hi > lo:
            f.tensor.copy_(torch.rand(dec.local_shape, dtype=torch.float64, device="cuda", generator=gen) * (hi - lo) + lo)
        fields[name] = f
    levels = [0, 1, 39, 78, 79]
    host_in = fields["in_field"].tensor[:, :, levels].cpu().numpy()
    host_cf = fields["coeff"].tensor[:, :, levels].cpu().numpy()
    ex = NativeHaloExchanger(dec, np.float64, comm, single_phase=single_phase)
    if single_phase:  # 2 I faces + 2 J faces of owned cells + 4 corners of 2 x 2
        assert ex.bytes_per_exchange == (2 * (2 * 1024) + 2 * (512 * 2) + 4 * 4) * 80 * 8
    origin = {n: dec.origin for n in fields}
    assert fused_apply(hd, dec, origin, fields, {"in_field": ex})
    torch.cuda.synchronize()
    want = np.zeros_like(host_in)
    wrapped = _wrap(host_in, h)
    R.hdiff(wrapped, want, host_cf, domain=(gd[0], gd[1], len(levels)))
    got = fields["out_field"].tensor[:, :, levels].cpu().numpy()
    assert np.array_equal(got[h:-h, h:-h], want[h:-h, h:-h])
    assert np.array_equal(fields["in_field"].tensor[:, :, levels].cpu().numpy(), wrapped)
    ii = torch.arange(dec.local_shape[0], dtype=torch.float64, device="cuda")[:, None, None]
    jj = torch.arange(dec.local_shape[1], dtype=torch.float64, device="cuda")[None, :, None]
    fields["in_field"].tensor.copy_((3.0 * ii + 5.0 * jj + 7.0).expand(dec.local_shape))
    assert fused_apply(hd, dec, origin, fields, {"in_field": ex})
    torch.cuda.synchronize()
    out, inp = fields["out_field"].tensor, fields["in_field"].tensor
    inner = (slice(h + 2, -(h + 2)), slice(h + 2, -(h + 2)), slice(None))
    assert torch.equal(out[inner], inp[inner])
    ex.close()


# (the 5-point cases are named by their schedule alone)
@pytest.mark.parametrize("stencil, schedule", [pytest.param(st, sc, id=sc if st == "lap5" else f"{st}-{sc}")
                                               for st in ("lap5", "hdiff")
                                               for sc in ("join", "chain", "swap", "swap-packed", "inline")])
def test_fused_laplacian_step_is_complete_in_stream_order_when_the_interior_is_longer(comm, stencil, schedule):
    """The other way round: a big interior next to small faces.  Whatever stream a schedule puts the interior kernel on (the
    side stream in "swap"), work the caller enqueues after the step on ITS stream -- here a copy of the result, no device
    synchronisation in between -- must see the whole result.  Both stencil families: one driver lays out their steps."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger

    dec = Decomposition((512, 512, 96), (1, 1), 0, 1 if stencil == "lap5" else 2, periodic=(False, True))
    inp = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
    out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
    ref = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
    inp.tensor.uniform_(-1, 1)
    ex = NativeHaloExchanger(dec, np.float64, comm).tune(schedule, 0)
    ex.exchange(inp)
    torch.cuda.synchronize()
    # the reference: the whole-domain kernel on the exchanged field
    if stencil == "lap5":
        lap = gtscript.stencil(backend="hip:mi300", definition=hip_templates.lap_notebook, dtypes={"T": np.float64})
        lap(inp=inp, out=ref, origin={"inp": dec.origin, "out": dec.origin}, domain=dec.local_domain)
        step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin)
    else:
        coeff = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
        coeff.tensor.uniform_(0, 0.5)
        hd = gtscript.stencil(backend="hip:mi300", definition=hip_templates.hdiff_limiter_field, dtypes={"T": np.float64})
        hd(in_field=inp, out_field=ref, coeff=coeff, origin={n: dec.origin for n in ("in_field", "out_field", "coeff")},
           domain=dec.local_domain)
        step = ex.make_dist_hdiff(inp, out, coeff, dec.origin, _lib.HDIFF_LIMITER)
    torch.cuda.synchronize()
    for attempt in range(5):
        out.tensor.zero_()
        step()
        last = out.tensor[:, :, -1].clone()  # stream-ordered after the step: the level the interior kernel writes LAST, first
        got = out.tensor.clone()
        torch.cuda.synchronize()
        assert torch.equal(last, ref.tensor[:, :, -1]), (schedule, attempt, int((last != ref.tensor[:, :, -1]).sum()))
        assert torch.equal(got, ref.tensor), (schedule, attempt, int((got != ref.tensor).sum()))
    # (the test sees a missing join: with GT4MI_PLAN_DEFER_JOIN the same copies differ in tens of thousands of points)
    ex.tune(defer_join=True)
    seen = 0
    for attempt in range(3):
        out.tensor.zero_()
        step()
        last = out.tensor[:, :, -1].clone()
        got = out.tensor.clone()
        ex.end()
        torch.cuda.synchronize()
        seen += int((last != ref.tensor[:, :, -1]).sum()) + int((got != ref.tensor).sum())
        assert torch.equal(out.tensor, ref.tensor)  # after the join everything is there
    # (a race the other way round: not an error, but then this test shows nothing; "join" and "inline" leave nothing to defer)
    if schedule not in ("join", "inline") and seen == 0:
        import warnings

        warnings.warn(f"schedule {schedule}: the copies enqueued before the deferred join happened to see the whole result")
    ex.close()


@pytest.mark.parametrize("schedule", ["join", "chain", "swap", "swap-packed", "inline"])
@pytest.mark.parametrize("stencil", ["lap5", "hdiff"])
def test_fused_steps_wait_for_the_exchange_when_the_interior_is_shorter(comm, stencil, schedule):
    """A flat, wide local domain: the interior kernel (a few rows) finishes long before the 1-2 MB faces have travelled, so a
    ring kernel that did not wait for the unpack would read the stale ghost rows.  (Round 3 briefly had exactly that: the
    join was skipped in the join schedule of gt4mi_dist_lap5_f64; the small domains of the other tests never showed it.)"""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from oracle import ref_numpy as R

    h = 1 if stencil == "lap5" else 2
    gd = (2048, 8, 96)
    dec = Decomposition(gd, (1, 1), 0, h, periodic=(False, True))
    rng = np.random.default_rng(31)
    host = rng.uniform(-1, 1, dec.local_shape)
    for attempt in range(3):
        inp = gt_storage.from_array(host, backend="hip:mi300", aligned_index=dec.origin)
        out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
        ex = NativeHaloExchanger(dec, np.float64, comm, single_phase=bool(attempt % 2)).tune(schedule, 0)
        wrapped = _wrap(host, h, False, True)
        want = np.zeros_like(host)
        if stencil == "lap5":
            step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin)
            R.laplacian(wrapped[h - 1:wrapped.shape[0] - h + 1, h - 1:wrapped.shape[1] - h + 1] if h > 1 else wrapped, want)
        else:
            coeff = gt_storage.from_array(np.full(dec.local_shape, 0.1), backend="hip:mi300", aligned_index=dec.origin)
            step = ex.make_dist_hdiff(inp, out, coeff, dec.origin, _lib.HDIFF_LIMITER)
            R.hdiff(wrapped, want, np.full(dec.local_shape, 0.1), domain=gd)
        step()
        torch.cuda.synchronize()
        assert np.array_equal(out.get(), want), (stencil, schedule, attempt)
        ex.close()


# ---- two REAL ranks on the one GPU of the box -------------------------------------------------------------------------
# RCCL refuses two ranks on one device, so the native plan cannot run here with a peer that is not the rank itself.  The
# torch transport can: two processes share GPU 0, the process group is gloo, the dense face buffers are staged through
# pinned host memory (HaloExchanger(stage_on_host=True)).  Everything else is the decomposed GPU path as an N-GPU job runs
# it -- scatter of a global field, HIP pack / unpack kernels, the kernel-library stencils on the interior and on the
# boundary strips, per-rank origins -- with neighbours that are OTHER processes.
def _two_rank_worker(rank: int, world: int, tmpdir: str, grid):
    """(run by tests/mp_util.run_ranks: the gloo group exists, the return value is this rank's report)"""
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import (Decomposition, HaloExchanger, overlapped_apply, scatter_global, sequential_apply)
    from oracle import ref_numpy as R

    rng = np.random.default_rng(4096)  # the same stream on every rank: the same global fields
    results = {}
    for name, h, gd in (("hdiff", 2, (150, 70, 5)), ("lap5", 1, (150, 70, 5))):
        glob = rng.uniform(-10, 10, (gd[0] + 2 * h, gd[1] + 2 * h, gd[2]))
        coeff = rng.uniform(0, 0.5, glob.shape)
        want = np.zeros_like(glob)
        if name == "hdiff":
            R.hdiff(glob, want, coeff, domain=gd)
            stencil = gtscript.stencil(backend="hip:mi300", definition=hip_templates.hdiff_limiter_field,
                                       dtypes={"T": np.float64}, device_sync=False)
            read, write = "in_field", "out_field"
        else:
            R.laplacian(glob, want)
            stencil = gtscript.stencil(backend="hip:mi300", definition=hip_templates.lap_notebook, dtypes={"T": np.float64},
                                       device_sync=False)
            read, write = "inp", "out"
        dec = Decomposition(gd, grid, rank, h)
        for form, apply in (("overlapped", overlapped_apply), ("sequential", sequential_apply)):
            for single_phase in (False, True):
                blk = scatter_global(glob, dec).copy()
                nb = dec.neighbours  # ghost cells that belong to the neighbour must come from the exchange
                if nb["W"] is not None:
                    blk[:h] = np.nan
                if nb["E"] is not None:
                    blk[-h:] = np.nan
                if nb["S"] is not None:
                    blk[:, :h] = np.nan
                if nb["N"] is not None:
                    blk[:, -h:] = np.nan
                args = {read: gt_storage.from_array(blk, backend="hip:mi300", aligned_index=dec.origin),
                        write: gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)}
                if name == "hdiff":
                    args["coeff"] = gt_storage.from_array(scatter_global(coeff, dec), backend="hip:mi300", aligned_index=dec.origin)
                origin = {n: dec.origin for n in args}
                ex = HaloExchanger(dec, torch.float64, torch.device("cuda", 0), single_phase=single_phase, stage_on_host=True)
                apply(stencil, dec, origin, args, {read: ex})
                torch.cuda.synchronize()
                assert np.array_equal(args[read].get(), scatter_global(glob, dec)), (name, form, "ghost cells")
                results[(name, form, single_phase)] = args[write].get()[h:-h, h:-h].copy()
        gathered = [None] * world
        dist.all_gather_object(gathered, (dec.global_slices(with_halo=False), {k: v for k, v in results.items() if k[0] == name}))
        if rank == 0:
            for key in gathered[0][1]:
                got = np.zeros_like(glob)
                for sl, res in gathered:
                    got[sl] = res[key]
                assert np.array_equal(got[h:-h, h:-h], want[h:-h, h:-h]), key
    return {"checked": len(results)}


@pytest.mark.multiprocess
@pytest.mark.parametrize("grid", [(1, 2), (2, 1)])
def test_two_processes_share_the_gpu_and_exchange_real_faces(grid, tmp_path):
    """World size 2 on the GPU: each rank owns half of a global field, its neighbour is ANOTHER process.  Horizontal diffusion
    (ghost depth 2, corners through either message table) and the Laplacian through the stencil-agnostic drivers; the
    assembled result equals the oracle on the undecomposed field bit for bit, and every rank's ghost cells equal the global
    field's values."""
    from mp_util import run_ranks

    reports = run_ranks(_two_rank_worker, 2, tmp_path, args=(grid,))
    assert [reports[r]["checked"] for r in (0, 1)] == [8, 8]




def _second_chance(test):
    """The tests below drive `bench.py` / the self-check through `torch.distributed.run` in a subprocess: rendezvous on a port
    found a moment earlier, a fresh RCCL communicator, deadlines.  One full-suite run in five showed one of them fail and
    never again in isolation; since the suite runs with -x, a single environmental hiccup there would hide every test
    after it -- so: a failed attempt is reported (warning), LOGGED (gpurun_out/retries.jsonl: the run's last test fails when the
    file is non-empty, tests/retry_log.py) and repeated ONCE."""
    import functools
    import warnings

    @functools.wraps(test)
    def wrapper(*args, **kwargs):
        try:
            return test(*args, **kwargs)
        except AssertionError as first:
            import retry_log

            # never free: the entry fails the run's last test (tests/test_zz_retries.py) unless GT4MI_ALLOW_RETRY=1
            retry_log.record(retry_log.current_test_id(test.__name__), str(first))
            warnings.warn(f"{test.__name__}: first attempt failed ({str(first)[:500]}); trying once more")
            return test(*args, **kwargs)

    return wrapper


@pytest.mark.multiprocess
@pytest.mark.parametrize("workload", ["lap512", "hdiff2048"])
@_second_chance
def test_bench_n_gpu_code_path_with_a_world_of_one(workload, tmp_path):
    """`bench.py` the way the driver launches it for N > 1 (torch.distributed.run, nccl process group), with a world of ONE rank
    forced onto the distributed code path (GT4MI_BENCH_FORCE_DISTRIBUTED=1): rendezvous, barriers and all-reduces on the
    device, the native communicator created through the broadcast of its id, the calibration of grid x message table x
    schedule x throttle, the informational steppers, and the keys the N > 1 line must carry.  Everything of that path
    except a message to another device."""
    import json
    import os
    import pathlib
    import socket
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, GT4MI_BENCH_FORCE_DISTRIBUTED="1")
    proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                           "--master-port", str(port), str(root / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2", "--full",
                           "--workload", workload], env=env, capture_output=True, text=True, timeout=900, cwd=str(root))
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]  # ONE JSON line on stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["unit"] == "GLUPS"
    assert line["rccl_nranks"] == 1 and line["rank_devices"] == [[0, 0]] and line["rccl_matches_n_gpus"] is True
    assert line["transport_fallback"] is False and line["config"]["transport"] == "native"
    assert line["config"]["calibration_ms_per_apply"] and "extra" in line
    verified = line["config"]["verified"]  # every calibrated form reproduced the exactly known outcome (distributed/selfcheck.py)
    assert verified["headline_form_correct_on_every_rank"] is True and verified["forms_rejected"] == 0
    assert verified["forms_checked"] >= len(line["config"]["calibration_ms_per_apply"]) + 2 and verified["ghost_cells_checked_on_rank_0"] == 0
    # the direct transport passed its canary (a child process per rank maps and stores first) and was calibrated beside RCCL
    assert line["config"]["direct_transport_canary"] is True and line["config"]["direct_transport_dropped_at"] is None
    table = line["config"]["calibration_ms_per_apply"]
    assert any(key.endswith("direct") for key in table)
    # what the SPECIFIED design (RCCL send/recv on a second stream) achieves next to the direct transport, at the top level; and
    # how much of the calibration the wall-clock budget allowed
    assert line["rccl_best_ms_per_apply"] == min(v for k, v in table.items() if not k.endswith("direct")) and line["rccl_best_form"] in table
    assert line["direct_best_ms_per_apply"] == min(v for k, v in table.items() if k.endswith("direct"))
    assert line["calibration_candidates_run"] >= len(table) and line["calibration_candidates_skipped_for_time"] >= 0
    # every process grid the calibration measured, with its per-apply time on each transport and the bytes of one face message per
    # neighbour: the first multi-device record shows whether a grid's big faces hid behind its interior
    grids = line["per_process_grid"]
    assert f"{config_grid(line)}" in grids and all(set(g["best_ms_per_apply"]) <= {"rccl", "direct"} and g["best_ms_per_apply"] for g in grids.values())
    mine = grids[config_grid(line)]
    assert mine["local_domain"] == line["config"]["local_domain"]
    assert (sum(mine["face_bytes_per_neighbour"].values()) > 0) == (config_grid(line) != "1x1")  # (a world of one has no faces)
    assert min(min(g["best_ms_per_apply"].values()) for g in grids.values()) == min(table.values())
    if workload == "lap512":
        assert {"timestep_glups", "timestep_ms_per_step", "pipelined_apply_glups"} <= set(line["extra"])
        assert line["config"]["mode"] == "apply" and line["config"]["halo_depth"] == 1
    assert "NATIVE RCCL TRANSPORT UNAVAILABLE" not in proc.stderr


@pytest.mark.multiprocess
@pytest.mark.parametrize("workload,phase", [("lap512", "calibration"), ("hdiff2048", "calibration"), ("lap512", "informational")])
@_second_chance
def test_bench_prints_what_it_measured_when_a_later_phase_hangs(workload, phase, tmp_path):
    """The first run on N > 1 devices tries forms that never ran between two devices.  Before it does, `bench.py` measures the
    plainest form (exchange, then one launch) by the contract; a phase that then overruns its deadline -- simulated here:
    GT4MI_BENCH_TEST_HANG -- ends the run with THAT line ("provisional", "deadline_exceeded"), status 0, instead of status 3
    and no line.  After the headline is measured, a hanging informational section costs only itself."""
    import json
    import os
    import pathlib
    import socket
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, GT4MI_BENCH_FORCE_DISTRIBUTED="1", GT4MI_BENCH_TEST_HANG=phase, GT4MI_BENCH_DEADLINE_SCALE="0.5")
    proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                           "--master-port", str(port), str(root / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2", "--full",
                           "--workload", workload], env=env, capture_output=True, text=True, timeout=900, cwd=str(root))
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["value"] > 0 and line["steps"] == 10 and line["warmup"] == 2 and line["roofline"]["frac"] > 0.3
    assert "a hang simulated for the tests" in line["deadline_exceeded"] and "deadline of phase" in proc.stderr
    assert line["rccl_nranks"] == 1 and line["transport_fallback"] is False
    if phase == "calibration":
        assert "sequential form" in line["provisional"] and line["config"]["transport"] == "native"
        assert "sequential form" in line["config"]["workload"]
    else:
        assert "provisional" not in line and line["config"]["calibration_ms_per_apply"]


@pytest.mark.parametrize("periodic,halo", [((True, True), 1), ((False, True), 1), ((True, True), 2)])
def test_form_check_accepts_the_fused_applies_and_sees_a_form_that_reads_ghost_cells_too_early(periodic, halo):
    """distributed.FormCheck (what bench.py runs on every rank before it trusts a form of the distributed apply): the fused
    applies pass on the self-loop; a form that skips the exchange, and one that computes the ring BEFORE the exchange has
    delivered (every ghost cell correct by the time anybody looks, the result not), are both seen."""
    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, FormCheck, NativeComm, NativeHaloExchanger

    dec = Decomposition((96, 40, 6), (1, 1), 0, halo=halo, periodic=periodic)
    new = lambda: gt_storage.zeros(dec.local_shape, np.float64, backend="hip:mi300", aligned_index=dec.origin)  # noqa: E731
    comm = NativeComm(rank=0, world_size=1)
    ex = NativeHaloExchanger(dec, np.float64, comm)
    if halo == 1:
        st = gtscript.stencil(backend="hip:mi300", definition=hip_templates.lap_notebook, dtypes={"T": np.float64})
        fr = st.freeze(origin={"inp": dec.origin, "out": dec.origin}, domain=dec.local_domain)
        local = lambda a, b: fr(inp=a, out=b)  # noqa: E731
    else:
        st = gtscript.stencil(backend="hip:mi300", definition=hip_templates.hdiff_limiter_field, dtypes={"T": np.float64})
        coeff = new()
        coeff.tensor.fill_(0.025)
        fr = st.freeze(origin={n: dec.origin for n in ("in_field", "out_field", "coeff")}, domain=dec.local_domain)
        local = lambda a, b: fr(in_field=a, out_field=b, coeff=coeff)  # noqa: E731
    chk = FormCheck(dec, new, local)
    assert chk.ghost_cells_to_fill > 0
    for schedule in ("join", "chain", "swap", "swap-packed"):
        ex.tune(schedule, 0)
        fused = (ex.make_dist_lap5(chk.probe, chk.out, dec.origin, dec.origin) if halo == 1 else
                 ex.make_dist_hdiff(chk.probe, chk.out, coeff, dec.origin, type(st)._gt_binding_.flags))
        chk.reset()
        fused()
        ex.end()
        assert chk.verdict()[0], (schedule, chk.verdict()[1])
        # ... and for consecutive epochs (each round's correct values differ from the last round's in every cell), the last one
        # next to an HBM-saturating background
        before = chk.epoch

        def run(fused=fused):
            fused()
            ex.end()

        ok, found = chk.check(run, rounds=3, loaded=1)
        assert ok and chk.epoch == before + 3 and "3 epochs, 1 of them under HBM load" in found, (schedule, found)
    # a receive side that hands out what the PREVIOUS exchange delivered (the round-3 defect of the direct transport): with a
    # probe that never changed this was the right answer in every round but a plan's first; with the epoch it is wrong everywhere
    import torch

    chk.reset()
    fused()
    ex.end()
    assert chk.verdict()[0]
    previous = chk.probe.tensor.clone()  # (the ghost cells of this epoch, as a stale receive buffer would hand them out next time)
    chk.reset()
    mine = torch.zeros_like(previous, dtype=torch.bool)
    h, (di, dj, _) = dec.halo, dec.local_domain
    mine[h:h + di, h:h + dj] = True
    chk.probe.tensor.copy_(torch.where(mine, chk.probe.tensor, previous))
    local(chk.probe, chk.out)
    ok, found = chk.verdict()
    assert not ok and f"[{chk.ghost_cells_to_fill} of them hold the previous epoch's value" in found and ", 0 points of the result" not in found
    chk.reset()  # no exchange at all
    local(chk.probe, chk.out)
    ok, found = chk.verdict()
    assert not ok and f"{chk.ghost_cells_to_fill} cells of the exchanged field differ" in found
    chk.reset()  # the kernel first, the exchange afterwards: every cell is right in the end, the ring of the result is not
    local(chk.probe, chk.out)
    ex.exchange(chk.probe)
    ok, found = chk.verdict()
    assert not ok and found.startswith("0 cells of the exchanged field differ") and ", 0 points of the result" not in found
    ex.close()


@pytest.mark.multiprocess
@_second_chance
def test_selfcheck_command_line_under_torchrun(tmp_path):
    """`python -m torch.distributed.run ... -m gt4py_amd.distributed`: the deployment check of the multi-GPU path
    (every transport, message table, fused step and schedule on exactly known fields, every rank's verdict gathered) -- here
    with a world of one rank, once bounded (nothing to exchange: the plumbing) and once periodic (every neighbour the rank
    itself)."""
    import os
    import pathlib
    import socket
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    for extra, checks in ((["--periodic", "--transport", "native"], 88), ([], 96)):
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
                               "127.0.0.1", "--master-port", str(port), "-m", "gt4py_amd.distributed", "--domain", "192", "96",
                               "6"] + extra, env=dict(os.environ, PYTHONPATH=str(root)), capture_output=True, text=True, timeout=600,
                              cwd=str(root))
        assert proc.returncode == 0, (proc.stdout[-2000:], proc.stderr[-2000:])
        lines = [ln for ln in proc.stdout.splitlines() if "ok on every rank" in ln or "WRONG" in ln]
        assert not any("WRONG" in ln for ln in lines), proc.stdout[-3000:]
        if "NOT AVAILABLE" in proc.stdout:  # (an environment without hipIpc / fine-grained memory: the RCCL checks remain)
            continue
        assert len(lines) == checks, proc.stdout[-3000:]
        assert "all correct" in proc.stdout
        assert any("fused swap-packed wg2" in ln for ln in lines) and any("halo 2" in ln and "fused chain" in ln for ln in lines)
        assert any("native/direct single-phase fused inline wg0" in ln for ln in lines)


@pytest.mark.parametrize("grid", [(4, 2), (1, 8)])
def test_tridiagonal_solve_decomposes_without_any_exchange_on_the_device(grid):
    """BASELINE configs[3] decomposed (ghost depth 0, no message): every rank's share through the
    drivers with an empty exchange table, the kernel-library solve underneath, == the oracle on the undecomposed fields,
    the in-place updates of ``sup`` / ``rhs`` included."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.distributed import Decomposition, overlapped_apply, sequential_apply
    from oracle import ref_numpy as R

    tri = gtscript.stencil(backend="hip:mi300", definition=hip_templates.tridiagonal_solver, dtypes={"T": np.float64}, device_sync=False)
    assert type(tri)._gt_binding_.family == "tridiag"
    rng = np.random.default_rng(7)
    gd = (70, 44, 61)
    glob = {"inf": rng.uniform(-1, 1, gd), "diag": rng.uniform(4, 5, gd), "sup": rng.uniform(-1, 1, gd), "rhs": rng.uniform(-10, 10, gd),
            "out": np.zeros(gd)}
    want = {k: v.copy() for k, v in glob.items()}
    R.tridiag(want["inf"], want["diag"], want["sup"], want["rhs"], want["out"])
    for apply in (overlapped_apply, sequential_apply):
        got = {k: np.full(gd, np.nan) for k in ("sup", "rhs", "out")}
        for rank in range(grid[0] * grid[1]):
            dec = Decomposition(gd, grid, rank, 0)
            sl = dec.global_slices(with_halo=False)
            args = {k: gt_storage.from_array(np.ascontiguousarray(v[sl]), backend="hip:mi300") for k, v in glob.items()}
            apply(tri, dec, {k: (0, 0, 0) for k in args}, args, {})
            torch.cuda.synchronize()
            for k in got:
                got[k][sl] = args[k].get()
        for k in got:
            assert np.array_equal(got[k], want[k]), (apply.__name__, k)


# ---- the direct transport: peer stores from the pack kernel (csrc/direct.hip.h) -----------------------------------------------
def _direct(ex):
    """Switch an exchanger to the direct transport -- or skip the test where the runtime lacks what it needs (fine-grained device
    memory, hipIpc): a capability of the environment, not of the code under test."""
    try:
        return ex.use_direct_transport()
    except RuntimeError as err:
        if "not available on every rank" in str(err):
            pytest.skip(str(err)[:300])
        raise


@pytest.mark.parametrize("single_phase", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("halo", [1, 2, 3])
@pytest.mark.parametrize("periodic", [(True, True), (False, True), (True, False)])
def test_direct_transport_exchange_on_the_self_loop(comm, periodic, halo, dtype, single_phase):
    """Every neighbour the rank itself: after the exchange (pack kernel -> my own receive buffers, flags, unpack kernel) the
    ghost cells hold the periodic wrap, for odd sizes (faces that are no whole 16-byte vectors) too, exchange after exchange
    (the flags count up, the buffers are reused), and RCCL can be switched back on."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger

    for gd in ((40, 36, 3), (131, 67, 5)):
        dec = Decomposition(gd, (1, 1), 0, halo, periodic=periodic)
        ex = _direct(NativeHaloExchanger(dec, dtype, comm, single_phase=single_phase))
        assert ex.transport == "direct"
        rng = np.random.default_rng(3)
        for repeat in range(4):
            host = rng.uniform(-1, 1, dec.local_shape).astype(dtype)
            dev = gt_storage.from_array(host, dtype, backend="hip:mi300", aligned_index=dec.origin)
            ex.exchange(dev)
            torch.cuda.synchronize()
            assert np.array_equal(dev.get(), _wrap(host, halo, *periodic)), (gd, repeat)
        status = ex.direct_status()
        assert status == {"timed_out": False, "exchanges": 4}
        ex.use_rccl_transport()
        dev = gt_storage.from_array(host, dtype, backend="hip:mi300", aligned_index=dec.origin)
        ex.exchange(dev)
        torch.cuda.synchronize()
        assert np.array_equal(dev.get(), _wrap(host, halo, *periodic))
        ex.close()


@pytest.mark.parametrize("fenced", [False, True])
@pytest.mark.parametrize("schedule", ["join", "chain", "swap", "swap-packed", "inline"])
@pytest.mark.parametrize("stencil", ["lap5", "hdiff"])
def test_fused_steps_on_the_direct_transport(comm, stencil, schedule, fenced):
    """The fused distributed steps with the faces pushed by the pack kernel: every schedule (also "inline": one stream, no
    event), both message tables, bit-identical to the oracle on the wrapped field and to the RCCL transport; and the flat wide
    domain whose interior is shorter than the exchange (a ring that did not wait for the unpack would read stale rows).
    ``fenced``: the same in the transport's fenced mode (GT4MI_PLAN_DIRECT_FENCED: a system-scope release before every flag is
    raised, an acquire behind every flag load) -- the rung between the default mode and RCCL on bench.py's ladder."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from oracle import ref_numpy as R

    h = 1 if stencil == "lap5" else 2
    for gd, periodic in (((130, 70, 4), (True, True)), ((300, 40, 4), (False, True)), ((2048, 8, 96), (False, True))):
        dec = Decomposition(gd, (1, 1), 0, h, periodic=periodic)
        rng = np.random.default_rng(31)
        host = rng.uniform(-1, 1, dec.local_shape)
        wrapped = _wrap(host, h, *periodic)
        want = np.zeros_like(host)
        coeff_host = np.full(dec.local_shape, 0.1)
        if stencil == "lap5":
            R.laplacian(wrapped, want)
        else:
            R.hdiff(wrapped, want, coeff_host, domain=gd)
        for single_phase in (False, True):
            inp = gt_storage.from_array(host, backend="hip:mi300", aligned_index=dec.origin)
            out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
            ex = _direct(NativeHaloExchanger(dec, np.float64, comm, single_phase=single_phase).tune(schedule, 0)).tune(direct_fenced=fenced)
            assert ex.direct_fenced is fenced
            if stencil == "lap5":
                step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin)
            else:
                coeff = gt_storage.from_array(coeff_host, backend="hip:mi300", aligned_index=dec.origin)
                step = ex.make_dist_hdiff(inp, out, coeff, dec.origin, _lib.HDIFF_LIMITER)
            for _ in range(3):
                step()
            ex.synchronize()  # (the consuming call: raises if a wait of the transport ran out of time)
            assert np.array_equal(out.get(), want), (gd, single_phase)
            assert np.array_equal(inp.get(), wrapped), (gd, single_phase)
            assert ex.direct_status()["timed_out"] is False
            ex.close()


@pytest.mark.parametrize("schedule", ["inline", "swap", "chain"])
@pytest.mark.parametrize("stencil", ["lap5", "hdiff"])
def test_a_neighbour_that_never_arrives_fails_the_direct_transport_hard(comm, stencil, schedule, monkeypatch):
    """VERDICT round 3, weak 7 / ADVICE: a device-side wait that runs out of time must not become silent garbage.  Pushes whose
    signals are lost (GT4MI_DIRECT_TEST_LOSE_SIGNALS when the plan is prepared: what a neighbour that never arrives looks like
    from the receiver's side), a short timeout: the call that ENQUEUES the failing exchange returns OK -- everything is
    asynchronous --, the waiting workgroups copy nothing (the ghost cells keep what they had: no stale or half-written face)
    and signal nothing, and the NEXT call on the plan that touches the exchange -- fused step, exchange, end() -- raises with
    status ERR_TIMEOUT, without anybody having polled; so does every call after it."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger

    monkeypatch.setenv("GT4MI_DIRECT_TEST_LOSE_SIGNALS", "1")
    h = 1 if stencil == "lap5" else 2
    dec = Decomposition((130, 70, 4), (1, 1), 0, h, periodic=(True, True))
    host = np.random.default_rng(5).uniform(-1, 1, dec.local_shape)
    host[:h], host[-h:], host[:, :h], host[:, -h:] = np.nan, np.nan, np.nan, np.nan
    inp = gt_storage.from_array(host, backend="hip:mi300", aligned_index=dec.origin)
    out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
    ex = _direct(NativeHaloExchanger(dec, np.float64, comm, single_phase=True).tune(schedule, 0, direct_timeout_ms=150))
    if stencil == "lap5":
        step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin)
    else:
        step = ex.make_dist_hdiff(inp, out, None, dec.origin, _lib.HDIFF_LIMITER, coeff_scalar=0.1)
    step()  # enqueued; the wait runs out on the device 150 ms later
    torch.cuda.synchronize()
    ghosts = inp.get()
    assert np.isnan(ghosts[:h]).all() and np.isnan(ghosts[-h:]).all() and np.isnan(ghosts[:, :h]).all() and np.isnan(ghosts[:, -h:]).all()
    for call in (step, lambda: ex.exchange(inp), ex.end, step):
        with pytest.raises(_lib.NativeError, match="ran out of time") as info:
            call()
        assert info.value.status == _lib.ERR_TIMEOUT
    assert ex.direct_status() == {"timed_out": True, "exchanges": 1}  # (the refused calls started nothing)
    ex.close()
    # an exchanger prepared without the lost signals works next to the failed one's remains
    monkeypatch.delenv("GT4MI_DIRECT_TEST_LOSE_SIGNALS")
    ex = _direct(NativeHaloExchanger(dec, np.float64, comm, single_phase=True).tune(schedule, 0, direct_timeout_ms=150))
    ex.exchange(inp)
    torch.cuda.synchronize()
    assert not np.isnan(inp.get()).any() and ex.direct_status()["timed_out"] is False
    ex.close()


def _two_rank_direct_worker(rank: int, world: int, tmpdir: str, grid, periodic, forms="all", cases=None, check_domain=(96, 80, 6)):
    """(run by tests/mp_util.run_ranks: the gloo group exists -- it only carries the descriptions of the pools and the results --,
    the return value is this rank's report)"""
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, FormCheck, NativeComm, NativeHaloExchanger, scatter_global
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from oracle import ref_numpy as R

    comm = NativeComm(rank=rank, world_size=world, rccl=False)  # RCCL cannot join two ranks on one device; no need to
    assert comm.info() == {"nranks": world, "rank": rank, "device": 0}
    rng = np.random.default_rng(4096)  # the same stream on every rank: the same global fields
    checked, log, edge_units_seen = 0, [], 0
    cases = cases or (("hdiff", 2, (150, 70, 5)), ("lap5", 1, (150, 70, 5)), ("lap5", 1, (131, 67, 3)))
    schedules = ("join", "chain", "swap", "swap-packed", "inline") if forms == "all" else tuple(forms.split(","))
    for name, h, gd in cases:
        shape = (gd[0] + 2 * h, gd[1] + 2 * h, gd[2])
        glob = rng.uniform(-10, 10, shape)
        coeff = rng.uniform(0, 0.5, shape)
        wrapped = glob.copy()  # the global field with its periodic wrap: what every rank's ghost cells must show
        if periodic[0]:
            wrapped[:h], wrapped[-h:] = wrapped[-2 * h:-h].copy(), wrapped[h:2 * h].copy()
        if periodic[1]:
            wrapped[:, :h], wrapped[:, -h:] = wrapped[:, -2 * h:-h].copy(), wrapped[:, h:2 * h].copy()
        want = np.zeros_like(glob)
        if name == "hdiff":
            R.hdiff(wrapped, want, coeff, domain=gd)
        else:
            R.laplacian(wrapped, want)
        dec = Decomposition(gd, grid, rank, h, periodic=periodic)
        results = {}
        for single_phase in (False, True):
            for schedule in schedules:
                blk = scatter_global(wrapped, dec).copy()
                mine = blk.copy()
                nb = dec.neighbours  # ghost cells that belong to a neighbour must come from the exchange
                for side, sl in (("W", np.s_[:h]), ("E", np.s_[-h:]), ("S", np.s_[:, :h]), ("N", np.s_[:, -h:])):
                    if nb[side] is not None:
                        mine[sl] = np.nan
                inp = gt_storage.from_array(mine, backend="hip:mi300", aligned_index=dec.origin)
                out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
                ex = NativeHaloExchanger(dec, np.float64, comm, single_phase=single_phase).tune(schedule, 0)
                with pytest.raises(RuntimeError, match="no RCCL behind it"):
                    ex.exchange(inp)  # this communicator cannot fall back to send/recv
                try:
                    ex.use_direct_transport()  # collective: the pools' descriptions travel over gloo, the faces never do
                except RuntimeError as err:  # (every rank raises together)
                    if "not available on every rank" not in str(err):
                        raise
                    return {"unavailable": str(err)[:300]}
                if __import__("os").environ.get("GT4MI_TEST_DIRECT_FENCED") == "1":
                    ex.tune(direct_fenced=True)
                if name == "hdiff":
                    cf = gt_storage.from_array(scatter_global(coeff, dec), backend="hip:mi300", aligned_index=dec.origin)
                    step = ex.make_dist_hdiff(inp, out, cf, dec.origin, _lib.HDIFF_LIMITER)
                else:
                    step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin)
                    # one receiving round (a single-phase table, or a grid cut along one axis) and a local width of whole
                    # 16-byte lanes: the unpack + ring are edge units -- on every rank, wherever it sits in the grid
                    # (an axis exchanges nothing when it is neither cut nor periodic)
                    one_round = single_phase or (grid[0] == 1 and not periodic[0]) or (grid[1] == 1 and not periodic[1])
                    want_units = one_round and dec.local_domain[0] % 2 == 0 and dec.local_domain[0] >= 4 and dec.local_domain[1] >= 2 and ex.sides != 0
                    assert ex.lap5_uses_edge_units(inp, out, dec.origin, dec.origin) == want_units, (name, gd, single_phase, dec.local_domain)
                    edge_units_seen += int(want_units)
                for _ in range(3):  # (the flags count up; the peer's buffers are reused)
                    step()
                torch.cuda.synchronize()
                status = ex.direct_status()
                wrong_ghosts = int((inp.get() != blk).sum())
                log.append({"case": [name, list(gd), single_phase, schedule], "status": status, "wrong_ghost_cells": wrong_ghosts})
                assert wrong_ghosts == 0, (name, schedule, single_phase, "ghost cells", wrong_ghosts, status)
                assert status["timed_out"] is False
                results[(single_phase, schedule)] = out.get()[h:-h, h:-h].copy()
                ex.close()  # collective on this transport: nobody unmaps a pool another rank still pushes into
                checked += 1
        gathered = [None] * world
        dist.all_gather_object(gathered, (dec.global_slices(with_halo=False), results))
        if rank == 0:
            for key in gathered[0][1]:
                got = np.zeros_like(glob)
                for sl, res in gathered:
                    got[sl] = res[key]
                assert np.array_equal(got[h:-h, h:-h], want[h:-h, h:-h]), (name, key)
    # the self-check bench.py runs on every form, here between two processes
    dec = Decomposition(tuple(check_domain), grid, rank, 1, periodic=periodic)
    lap = gtscript.stencil(backend="hip:mi300", definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    fr = lap.freeze(origin={"inp": dec.origin, "out": dec.origin}, domain=dec.local_domain)
    chk = FormCheck(dec, lambda: gt_storage.zeros(dec.local_shape, np.float64, backend="hip:mi300", aligned_index=dec.origin),
                    lambda a, b: fr(inp=a, out=b))
    ex = NativeHaloExchanger(dec, np.float64, comm, single_phase=True).tune("inline", 0).use_direct_transport()
    fused = ex.make_dist_lap5(chk.probe, chk.out, dec.origin, dec.origin)
    import os

    verdicts = []
    if os.environ.get("GT4MI_TEST_DIRECT_FENCED") == "1":
        ex.tune(direct_fenced=True)
    # EVERY round is sensitive: the probe carries an epoch (selfcheck.py), so the payload the previous round left in the receive
    # buffers is wrong in every cell; both ranks launch together (the receiver's unpack meets the sender's push in flight), and
    # every other round runs next to an HBM-saturating background (GT4MI_TEST_VERDICT_LOAD=all / none: every / no round)
    load = os.environ.get("GT4MI_TEST_VERDICT_LOAD", "alternate")
    for n in range(int(os.environ.get("GT4MI_TEST_VERDICT_ROUNDS", "8"))):
        loaded = 1 if load == "all" or (load == "alternate" and n % 2 == 1) else 0
        verdicts.append(list(chk.check(fused, rounds=1, loaded=loaded, before_run=dist.barrier)))
    status = ex.direct_status()
    ex.close()
    comm.close()
    failed = [(n, v[1]) for n, v in enumerate(verdicts) if not v[0]]
    if os.environ.get("GT4MI_TEST_VERDICT_KEEP_GOING") != "1":  # (scripts/two_rank_direct_loop.py counts the failed rounds itself)
        assert not failed, (f"rank {rank}: {len(failed)} of {len(verdicts)} self-check rounds failed", failed[:3], status)
    return {"checked": checked, "verdicts": verdicts, "status": status, "log": log, "edge_unit_cases": edge_units_seen}


@pytest.mark.multiprocess
@pytest.mark.parametrize("grid,periodic", [((1, 2), (False, False)), ((2, 1), (False, False)), ((1, 2), (True, True)), ((2, 1), (True, True))])
def test_two_processes_push_faces_into_each_other_on_one_gpu(grid, periodic, tmp_path):
    """TWO REAL RANKS of the native path on the one device of the box -- what RCCL refuses to do.  Each process exports its pool
    of flag words and receive buffers (hipIpcGetMemHandle) and maps the other's (hipIpcOpenMemHandle); the pack kernel of one
    process stores its faces into the OTHER process's memory and raises the flag there, the other's unpack kernel waits for
    it.  Horizontal diffusion (ghost depth 2, corners) and the Laplacian, every schedule of the fused steps, both message
    tables, bounded and periodic (then each rank is also its own neighbour along the uncut axis, and the same peer twice
    along the cut one); the assembled results equal the oracle on the undecomposed field, every rank's ghost cells the global
    field's values, and no wait ever times out.  Every rank reports (tests/mp_util.py)."""
    from mp_util import run_ranks

    reports = run_ranks(_two_rank_direct_worker, 2, tmp_path, args=(grid, periodic))
    if any("unavailable" in reports[r] for r in (0, 1)):  # no hipIpc / fine-grained memory here: the environment's, not the code's
        pytest.skip(str([reports[r].get("unavailable") for r in (0, 1)]))
    assert [reports[r]["checked"] for r in (0, 1)] == [30, 30]
    assert all(not reports[r]["status"]["timed_out"] for r in (0, 1))
    assert all(len(reports[r]["verdicts"]) == 8 and all(v[0] for v in reports[r]["verdicts"]) for r in (0, 1))  # 8 epochs, 4 under load


@pytest.mark.multiprocess
@pytest.mark.parametrize("grid,periodic", [((1, 2), (True, True)), ((2, 1), (False, False))])
def test_two_processes_push_faces_into_each_other_in_fenced_mode(grid, periodic, tmp_path, monkeypatch):
    """The same two real ranks on the one device with the direct transport in its FENCED mode (GT4MI_PLAN_DIRECT_FENCED): a
    system-scope release in front of every flag add, an acquire behind every flag load, in the stand-alone pack / unpack kernels,
    in the push that rides in the interior's launch and in the edge units.  Same oracle, same epoch-stamped self-check."""
    from mp_util import run_ranks

    monkeypatch.setenv("GT4MI_TEST_DIRECT_FENCED", "1")
    reports = run_ranks(_two_rank_direct_worker, 2, tmp_path, args=(grid, periodic, "inline,swap,chain"))
    if any("unavailable" in reports[r] for r in (0, 1)):
        pytest.skip(str([reports[r].get("unavailable") for r in (0, 1)]))
    assert [reports[r]["checked"] for r in (0, 1)] == [18, 18]
    assert all(not reports[r]["status"]["timed_out"] and all(v[0] for v in reports[r]["verdicts"]) for r in (0, 1))


def test_closing_a_failed_plan_does_not_wait_for_a_neighbour_that_is_gone(comm, monkeypatch):
    """`close()` of an exchanger that is connected to other ranks is collective -- and after GT4MI_ERR_TIMEOUT the
    neighbour that never arrived may be gone for good, so that collective may never complete.  A FAILED plan offers the round for
    a bounded time only, then leaks its pool (with a warning) instead of hanging; `synchronize()` is the consuming call that
    raises where a bare device synchronise would have returned incomplete ghost cells without a word."""
    import threading
    import time

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger

    monkeypatch.setenv("GT4MI_DIRECT_TEST_LOSE_SIGNALS", "1")
    dec = Decomposition((66, 40, 3), (1, 1), 0, 1, periodic=(True, True))
    inp = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
    ex = _direct(NativeHaloExchanger(dec, np.float64, comm).tune(direct_timeout_ms=100))
    ex.exchange(inp)  # returns OK: everything is asynchronous
    with pytest.raises(_lib.NativeError, match="ran out of time") as info:
        ex.synchronize()
    assert info.value.status == _lib.ERR_TIMEOUT
    gone = threading.Event()
    ex._close_round = lambda obj: gone.wait(60)  # (as if connected to a rank that no longer answers)
    ex.failed_close_seconds = 0.5
    t0 = time.monotonic()
    with pytest.warns(RuntimeWarning, match="the pool is leaked"):
        ex.close()
    assert time.monotonic() - t0 < 10.0
    gone.set()
    with pytest.raises(_lib.NativeError):  # a closed exchanger's plan is NULL: an error, never a crash
        ex.exchange(inp)
    # a healthy plan's close() still meets the others
    monkeypatch.delenv("GT4MI_DIRECT_TEST_LOSE_SIGNALS")
    ex = _direct(NativeHaloExchanger(dec, np.float64, comm))
    ex.exchange(inp)
    ex.synchronize()
    met = []
    ex._close_round = met.append
    ex.close()
    assert met == [("closing", 0)]


@pytest.mark.multiprocess
@pytest.mark.parametrize("grid,periodic", [((4, 2), (False, False)), ((2, 4), (True, True)), ((1, 8), (False, False))])
def test_eight_processes_on_one_gpu_exchange_faces_on_the_grids_of_an_eight_gpu_node(grid, periodic, tmp_path, monkeypatch):
    """EIGHT REAL RANKS of the native path on the one device of the box: the process grids an 8-GPU node would run -- 4 x 2 (the
    north star's; interior ranks have all four neighbours and, in the single-phase table, four diagonal ones), 2 x 4 periodic
    (every rank has every neighbour; along I the same peer twice), 1 x 8 -- with every pool mapped by its neighbours over hipIpc
    and every face pushed into ANOTHER process's memory.  What no test on this box could show before: ranks in every position
    of a grid (corner, edge, interior: every subset of sides, corner boxes to diagonal neighbours) running the fused
    Laplacian step -- one launch with its edge units where the local width allows it -- and the fused horizontal diffusion
    against each other.  The assembled results equal the oracle on the undecomposed field bit for bit, every rank's ghost cells
    the global field's values, the self-check passes on every rank, no wait times out.  (What it cannot show: the same stores
    crossing xGMI.)"""
    from mp_util import run_ranks

    monkeypatch.setenv("GT4MI_DIRECT_TIMEOUT_MS", "240000")  # (eight processes share ONE device's hardware queues: see the canary test)
    # local widths 2 * 76 / 4 = 38 ... : multiples of the 16-byte lane on every rank (the edge units take part) and one case where
    # they are not (131 / 4: the older launches)
    cases = (("hdiff", 2, (152, 72, 5)), ("lap5", 1, (152, 72, 5)), ("lap5", 1, (520, 136, 9)), ("lap5", 1, (131, 67, 3)))
    if grid == (1, 8):
        cases = (("hdiff", 2, (152, 72, 5)), ("lap5", 1, (152, 72, 5)), ("lap5", 1, (520, 136, 9)))
    reports = run_ranks(_two_rank_direct_worker, 8, tmp_path, args=(grid, periodic, "inline,swap", cases, (192, 160, 6)), timeout=900)
    if any("unavailable" in reports[r] for r in range(8)):
        pytest.skip(str([reports[r].get("unavailable") for r in range(8)]))
    assert [reports[r]["checked"] for r in range(8)] == [len(cases) * 2 * 2] * 8
    assert all(not reports[r]["status"]["timed_out"] and all(v[0] for v in reports[r]["verdicts"]) for r in range(8))
    # ... and the one-launch form with its edge units really ran on EVERY rank (corner, edge and interior positions alike) for
    # the two Laplacian cases whose local widths allow it: both schedules, with the single-phase table (on 1 x 8: both tables)
    from gt4py_amd.distributed import Decomposition

    def expected(rank):
        n = 0
        for name, h, gd in cases:
            di = Decomposition(gd, grid, rank, h, periodic=periodic).local_domain[0]
            tables = 2 if (grid[0] == 1 and not periodic[0]) or (grid[1] == 1 and not periodic[1]) else 1  # (one round with either table?)
            n += 2 * tables if name == "lap5" and di % 2 == 0 and di >= 4 else 0  # two schedules
        return n

    assert [reports[r]["edge_unit_cases"] for r in range(8)] == [expected(r) for r in range(8)] and min(expected(r) for r in range(8)) >= 4


@pytest.mark.multiprocess
@pytest.mark.parametrize("workload,ranks", [("lap512", 8), ("lap512", 4), ("hdiff2048", 8)])  # (both workloads on a 32-level slab: see bench.py, GT4MI_BENCH_ONE_DEVICE)
@_second_chance
def test_bench_n_gpu_code_path_with_real_ranks_on_one_device(workload, ranks, tmp_path):
    """`bench.py` exactly as the driver launches it for N > 1 -- `torch.distributed.run --nproc-per-node N bench.py --gpus N` --
    with N REAL ranks, all on the one device of the box (GT4MI_BENCH_ONE_DEVICE=1: the process group is gloo, the faces travel
    over the direct transport between the processes; RCCL refuses ranks that share a device).  A rehearsal of the control flow,
    never a measurement: every collective of the program with more than one participant, the provisional sequential form, the
    budgeted best-first calibration over every process grid of N ranks with the agreement on failures, the self-check of every
    form on every rank, the headline loop between barriers, the informational sections, the gathered proof -- and ONE JSON line
    with the keys an N-GPU line carries.  (The Laplacian is cut to a slab of 32 levels here: ranks that wait for each other share
    the device's wave slots, see bench.py.)"""
    import json
    import os
    import pathlib
    import socket
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, GT4MI_BENCH_ONE_DEVICE="1", GT4MI_BENCH_CALIBRATION_SECONDS="20", GT4MI_BENCH_DIRECT_CALIBRATION_SECONDS="30",
               GT4MI_BENCH_INFORMATIONAL_SECONDS="10", GT4MI_BENCH_DIRECT_TIMEOUT_MS="60000")
    proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
                           "127.0.0.1", "--master-port", str(port), str(root / "bench.py"), "--gpus", str(ranks), "--steps", "10", "--warmup",
                           "2", "--full", "--workload", workload], env=env, capture_output=True, text=True, timeout=1200, cwd=str(root))
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]  # ONE JSON line, from rank 0
    line = json.loads(lines[0])
    config = line["config"]
    assert line["n_gpus"] == ranks and line["value"] > 0 and line["steps"] == 10 and "provisional" not in line and "deadline_exceeded" not in line
    assert line["rccl_nranks"] == ranks and line["rank_devices"] == [[r, 0] for r in range(ranks)] and line["transport_fallback"] is False
    assert config["transport"] == "native" and config["verified"]["headline_form_correct_on_every_rank"] is True
    table = config["calibration_ms_per_apply"]
    assert table and all(key.endswith("_direct") for key in table) and line["direct_best_ms_per_apply"] == min(table.values())
    assert line["rccl_best_ms_per_apply"] is None and line["calibration_candidates_run"] >= len(table)
    if workload == "lap512":
        grids = {key.split("_")[0] for key in table}  # every process grid of N ranks took part (budget permitting: at least two)
        assert len(grids) >= 2 and f"1x{ranks}" in grids and config["decomposition"] in grids
        assert config["halo_transport"].startswith("direct")
    else:
        # BASELINE.json configs[4]'s control flow with 8 REAL ranks: the 4 x 2 grid the north star names, every rank's share
        # 512 x 1024 (x 32 levels here), a fused form of the direct transport as the headline
        assert config["decomposition"] == "4x2" and config["local_domain"][:2] == [512, 1024] and config["grid"][:2] == [2048, 2048]
        assert config["apply_form"].startswith("fused_") and config["apply_form"].endswith("_direct")
    # every form was checked on consecutive epochs of the probe (the last one under HBM load) and the transport stayed in its
    # default mode: nothing stepped down the ladder
    assert config["verified"]["epochs_per_form"] >= 3 and line["direct_transport_mode"] == "direct" and line["direct_transport_ladder"] == []
    assert "NATIVE RCCL TRANSPORT UNAVAILABLE" not in proc.stderr


@pytest.mark.multiprocess
@_second_chance
def test_the_canary_of_bench_with_eight_ranks_on_one_device(tmp_path):
    """What `bench.py` starts on every rank of an N-GPU run before it trusts the direct transport (`direct_canary`): the
    self-check of the multi-GPU path restricted to that transport -- `python -m gt4py_amd.distributed --transport direct`, its
    own gloo group met through a file -- here as EIGHT processes on the one device: the process grids `choose_process_grid`
    returns for 8 ranks, ghost depths 1 and 2, both message tables, the sequential form and every schedule of the fused steps,
    each checked on exactly known fields on every rank; rank 0 prints the table, every process ends with status 0."""
    import os
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    base = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC_")}
    # (eight processes with a handful of streams each oversubscribe the ONE device's hardware queues: the driver then time-slices
    # them, and a kernel that waits for a flag may wait for its sender's turn -- seen once in 41 runs as 30-s waits running out
    # right after the eight-process tests above had ended; an 8-GPU node has a device per rank)
    base["GT4MI_DIRECT_TIMEOUT_MS"] = "240000"
    import shutil
    import time

    shutil.rmtree(tmp_path / "rendezvous", ignore_errors=True)
    if (tmp_path / "rendezvous").exists():
        (tmp_path / "rendezvous").unlink()
    time.sleep(3.0)  # (the processes of the tests before this one are still handing their queues back)
    procs = []
    for rank in range(8):
        env = dict(base, GT4MI_RENDEZVOUS_FILE=str(tmp_path / "rendezvous"), RANK=str(rank), WORLD_SIZE="8", LOCAL_RANK="0",
                   PYTHONPATH=str(root) + os.pathsep + base.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "gt4py_amd.distributed", "--transport", "direct", "--domain", "256", "192", "8"],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=str(root)))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=600))
        except subprocess.TimeoutExpired:
            for q in procs:  # exactly the processes started above
                q.kill()
            pytest.fail("the self-check of the direct transport did not finish on 8 ranks within 600 s")
    wrong = [ln[:700] for ln in outs[0][0].splitlines() if "WRONG" in ln or "FAILED" in ln]
    assert [p.returncode for p in procs] == [0] * 8, "\n".join(wrong[:12]) + "\n" + "\n".join(
        f"rank {r}: {e[-400:]}" for r, (o, e) in enumerate(outs) if procs[r].returncode != 0)
    table = outs[0][0]
    assert "checks x 8 rank(s): all correct" in table and "WRONG" not in table
    assert "halo 1 grid 4x2 native/direct single-phase fused inline wg0" in table and "halo 2 grid 4x2 native/direct two-phase fused chain wg2" in table


@pytest.mark.multiprocess
def test_bench_drops_a_direct_transport_that_loses_its_signals(tmp_path):
    """A direct transport whose pushes never raise the receiver's flags (GT4MI_DIRECT_TEST_LOSE_SIGNALS: what a broken link looks
    like): the receiver's waits run out of time, the plan fails HARD (the next call on it raises ERR_TIMEOUT), `bench.py` drops
    the form and every later direct form, and the line is measured on RCCL -- slower to find out, never wrong."""
    import json
    import os
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    env = dict(os.environ, GT4MI_DIRECT_TEST_LOSE_SIGNALS="1", GT4MI_BENCH_TIMESTEP="0", GT4MI_BENCH_DIRECT_TIMEOUT_MS="250")
    proc = subprocess.run([sys.executable, str(root / "bench.py"), "--dist-selfloop", "--selfloop-grid", "1x8", "--steps", "10", "--warmup", "2"],
                          env=env, capture_output=True, text=True, timeout=600, cwd=str(root))
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    config = line["config"]
    assert config["halo_transport"].startswith("rccl") and config["direct_transport_dropped_at"].endswith("_direct")
    assert config["verified"]["headline_form_correct_on_every_rank"] is True
    assert not any(key.endswith("_direct") for key in config["calibration_ms_per_apply"])
    assert line["calibration_candidates_failed"] == [config["direct_transport_dropped_at"]] and line["direct_best_ms_per_apply"] is None
    assert line["rccl_best_ms_per_apply"] == min(config["calibration_ms_per_apply"].values())
    assert "calibration candidate failed" in proc.stderr and "ran out of time" in proc.stderr
    # ... by way of the fenced mode, which loses its signals just the same: both rungs of the ladder are in the line
    assert line["direct_transport_mode"] == config["direct_transport_mode"] == "rccl"
    assert [(st["from"], st["to"]) for st in line["direct_transport_ladder"]] == [("direct", "direct-fenced"), ("direct-fenced", "rccl")]
    assert line["calibration_candidates_failed_unfenced"] == [line["direct_transport_ladder"][0]["at"]]


@pytest.mark.multiprocess
def test_bench_steps_down_to_the_fenced_direct_transport_when_the_default_mode_fails(tmp_path):
    """The fall-back ladder direct -> direct-fenced -> rccl, fault injected: GT4MI_DIRECT_TEST_LOSE_SIGNALS=2
    loses the pushes' signals only while a plan is NOT in fenced mode -- a transport whose default ordering does not hold on
    these links and whose fenced mode does.  The first direct form fails (its waits run out of time, the plan fails hard),
    every rank steps down, what the default mode measured is discarded, the direct stage runs again with fences -- and the
    headline is a fenced direct form, checked on consecutive epochs like every other."""
    import json
    import os
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    env = dict(os.environ, GT4MI_DIRECT_TEST_LOSE_SIGNALS="2", GT4MI_BENCH_TIMESTEP="0", GT4MI_BENCH_DIRECT_TIMEOUT_MS="250",
               GT4MI_BENCH_CALIBRATION_SECONDS="15", GT4MI_BENCH_DIRECT_CALIBRATION_SECONDS="30")
    proc = subprocess.run([sys.executable, str(root / "bench.py"), "--dist-selfloop", "--selfloop-grid", "1x8", "--steps", "10", "--warmup", "2"],
                          env=env, capture_output=True, text=True, timeout=600, cwd=str(root))
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    config = line["config"]
    assert line["direct_transport_mode"] == config["direct_transport_mode"] == "direct-fenced" and config["direct_transport_dropped_at"] is None
    assert [(st["from"], st["to"]) for st in line["direct_transport_ladder"]] == [("direct", "direct-fenced")]
    assert line["calibration_candidates_failed"] == [] and line["calibration_candidates_failed_unfenced"] == [line["direct_transport_ladder"][0]["at"]]
    table = config["calibration_ms_per_apply"]
    assert any(key.endswith("_direct") for key in table) and line["direct_best_ms_per_apply"] == min(v for k, v in table.items() if k.endswith("_direct"))
    assert config["verified"]["headline_form_correct_on_every_rank"] is True and config["verified"]["epochs_per_form"] >= 3
    assert "steps down direct -> direct-fenced" in proc.stderr and "ran out of time" in proc.stderr


def test_fused_launches_of_the_direct_transport_on_random_shapes(comm):
    """Random local domains through the ONE launch of the inline schedule (push | interior | edge units, lap5_edge.hip.h) and --
    where the shape or the message table rules it out -- its fall-backs: widths that are no multiple of the tile or of the
    vector, two or three rows, one to twenty levels, every combination of periodic axes, both message tables, all four expressions.
    Bit-identical to the whole-domain kernel on the wrapped field; the exchanged field equals the wrap."""
    import ctypes

    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from gt4py_amd.distributed.native import _field_struct

    lib = _lib.load()
    rng = np.random.default_rng(2718)
    for case in range(40):
        di = int(rng.choice([2, 6, 30, 64, 126, 128, 130, 256, 258, 384, 514, 640]))
        dj = int(rng.choice([2, 3, 4, 9, 33]))
        dk = int(rng.choice([1, 3, 7, 8, 9, 16, 20]))
        periodic = [(False, True), (True, True), (True, False), (False, True)][case % 4]
        variant = case % 4
        dec = Decomposition((di, dj, dk), (1, 1), 0, 1, periodic=periodic)
        host = rng.uniform(-1, 1, dec.local_shape)
        wrapped = _wrap(host, 1, *periodic)
        inp = gt_storage.from_array(host, backend="hip:mi300", aligned_index=dec.origin)
        out = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
        ref = gt_storage.zeros(dec.local_shape, backend="hip:mi300", aligned_index=dec.origin)
        ex = _direct(NativeHaloExchanger(dec, np.float64, comm, single_phase=bool(case % 3 == 0)).tune("inline", 0))
        step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin, variant)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        assert np.array_equal(inp.get(), wrapped), (case, di, dj, dk, periodic)
        fi, fr = _field_struct(inp, dec.origin), _field_struct(ref, dec.origin)
        _lib.check("gt4mi_lap5_f64", lib.gt4mi_lap5_f64(_lib.domain3(dec.local_domain), ctypes.byref(fi), ctypes.byref(fr), variant, 0,
                                                        torch.cuda.current_stream().cuda_stream, None))
        torch.cuda.synchronize()
        assert np.array_equal(out.get(), ref.get()), (case, di, dj, dk, periodic, variant)
        assert ex.direct_status()["timed_out"] is False
        ex.close()


@pytest.mark.parametrize("transport", ["rccl", "direct"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_edge_units_on_random_shapes_every_schedule_and_side(comm, transport, dtype):
    """The unpack + ring of a distributed 5-point step as wave-sized units that read the receive buffers themselves
    (csrc/lap5_edge.hip.h: column units for W / E faces, row units for S / N, copies for the corner boxes), as a kernel of its
    own behind the send/recv kernel (RCCL) or the pushes (direct), and as the tail of the one launch of the inline schedule:
    random widths (multiples of the 16-byte lane or not: then the older launches run), 2 ... 70 rows, 1 ... 21 levels -- fewer,
    as many and more than a unit takes --, every combination of periodic axes (W / E only, S / N only, all four with the corner
    boxes of the single-phase table), every schedule, all four expressions, fp64 and fp32 (literal precision 64 and 32).
    Bit-identical to the whole-domain kernel on the wrapped field; the exchanged field equals the wrap; three applies in a row
    (the counters of the units wrap, the flags count on)."""
    import ctypes

    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib
    from gt4py_amd.distributed import Decomposition, NativeHaloExchanger
    from gt4py_amd.distributed.native import _field_struct

    lib = _lib.load()
    rng = np.random.default_rng(1618 if transport == "rccl" else 3141)
    f32 = np.dtype(dtype) == np.float32
    import os

    schedules = ["join", "chain", "swap", "swap-packed", "inline"]
    units = 0
    cases = int(os.environ.get("GT4MI_EDGE_CASES", "60"))  # (campaigns: profiles/r4_edge_units_campaign.log)
    for case in range(cases):
        di = int(rng.choice([4, 8, 30, 33, 64, 126, 128, 129, 132, 256, 260, 384, 516, 640, 1024]))
        dj = int(rng.choice([2, 3, 4, 9, 33, 64, 65, 70]))
        dk = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 21]))
        if case >= 60:  # (campaigns: any even or odd width, any height)
            di, dj = int(rng.integers(4, 700)), int(rng.integers(2, 140))
        periodic = [(False, True), (True, True), (True, False)][case % 3]
        variant, schedule = case % 4, schedules[(case + case // 5) % 5]
        flags = _lib.LAP_LITERAL_F32 if (f32 and case % 2) else 0
        dec = Decomposition((di, dj, dk), (1, 1), 0, 1, periodic=periodic)
        host = rng.uniform(-1, 1, dec.local_shape).astype(dtype)
        wrapped = _wrap(host, 1, *periodic)
        inp = gt_storage.from_array(host, dtype, backend="hip:mi300", aligned_index=dec.origin)
        out = gt_storage.zeros(dec.local_shape, dtype, backend="hip:mi300", aligned_index=dec.origin)
        ref = gt_storage.zeros(dec.local_shape, dtype, backend="hip:mi300", aligned_index=dec.origin)
        # (single-phase: one round -- the units take part; two-phase with both axes cut: two rounds -- the older launches)
        ex = NativeHaloExchanger(dec, dtype, comm, single_phase=bool(case % 4 != 3)).tune(schedule, 0)
        if transport == "direct":
            _direct(ex)
        step = ex.make_dist_lap5(inp, out, dec.origin, dec.origin, variant, flags=flags)
        vec = 16 // np.dtype(dtype).itemsize
        one_round = bool(case % 4 != 3) or not all(periodic)
        units += int(ex.lap5_uses_edge_units(inp, out, dec.origin, dec.origin))
        assert ex.lap5_uses_edge_units(inp, out, dec.origin, dec.origin) == (one_round and di % vec == 0 and di >= 2 * vec), (di, dj, dk, periodic, case)
        for _ in range(3):
            step()
            ex.end()
        torch.cuda.synchronize()
        what = (case, di, dj, dk, periodic, variant, schedule, transport)
        assert np.array_equal(inp.get(), wrapped), what
        fi, fr = _field_struct(inp, dec.origin), _field_struct(ref, dec.origin)
        if f32:
            _lib.check("gt4mi_lap5_f32", lib.gt4mi_lap5_f32(_lib.domain3(dec.local_domain), ctypes.byref(fi), ctypes.byref(fr), variant, flags,
                                                            torch.cuda.current_stream().cuda_stream, None))
        else:
            _lib.check("gt4mi_lap5_f64", lib.gt4mi_lap5_f64(_lib.domain3(dec.local_domain), ctypes.byref(fi), ctypes.byref(fr), variant, 0,
                                                            torch.cuda.current_stream().cuda_stream, None))
        torch.cuda.synchronize()
        assert np.array_equal(out.get(), ref.get()), what
        if transport == "direct":
            assert ex.direct_status()["timed_out"] is False
        ex.close()
    assert units >= 25  # (most cases take the units; the others -- two receiving rounds, odd widths -- the older launches)


@pytest.mark.multiprocess
@_second_chance
def test_bench_keeps_to_rccl_when_the_canary_of_the_direct_transport_fails(tmp_path):
    """On more than one rank `bench.py` lets a CHILD process per rank try the direct transport first (it maps another process's
    memory and stores into it: a fault there must end a child, not the run).  A canary that fails on any rank -- simulated --
    takes the direct transport out of every calibration; the line is measured on RCCL and says so."""
    import json
    import os
    import pathlib
    import socket
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, GT4MI_BENCH_FORCE_DISTRIBUTED="1", GT4MI_BENCH_TEST_CANARY_FAILS="1", GT4MI_BENCH_TIMESTEP="0")
    proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                           "--master-port", str(port), str(root / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2"],
                          env=env, capture_output=True, text=True, timeout=900, cwd=str(root))
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    config = line["config"]
    assert config["direct_transport_canary"] is False and config["halo_transport"].startswith("rccl")
    assert config["calibration_ms_per_apply"] and not any(key.endswith("direct") for key in config["calibration_ms_per_apply"])
    assert "did not pass its canary" in proc.stderr and line["transport_fallback"] is False
    # both rungs were tried in child processes (the default mode, then the fenced one) before the transport was given up
    assert line["direct_transport_mode"] == "rccl" and [st["at"] for st in line["direct_transport_ladder"]] == ["canary", "canary (fenced)"]


@pytest.mark.multiprocess
@_second_chance
def test_bench_uses_the_fenced_direct_transport_when_only_the_default_mode_fails_its_canary(tmp_path):
    """The canary's own ladder: the children of the default mode fail (simulated), the children of the FENCED mode run for real
    -- every form of the direct transport on consecutive epochs, the one-stream forms for many more under HBM load -- and pass:
    the calibration goes on with the direct transport in fenced mode on every rank, and the line says so."""
    import json
    import os
    import pathlib
    import socket
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, GT4MI_BENCH_FORCE_DISTRIBUTED="1", GT4MI_BENCH_TEST_CANARY_FAILS="unfenced", GT4MI_BENCH_TIMESTEP="0",
               GT4MI_BENCH_CALIBRATION_SECONDS="15", GT4MI_BENCH_DIRECT_CALIBRATION_SECONDS="20", GT4MI_BENCH_CANARY_EPOCHS="40")
    proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                           "--master-port", str(port), str(root / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2"],
                          env=env, capture_output=True, text=True, timeout=900, cwd=str(root))
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][-1])
    config = line["config"]
    assert config["direct_transport_canary"] is True and line["direct_transport_mode"] == "direct-fenced"
    assert [(st["from"], st["to"], st["at"]) for st in line["direct_transport_ladder"]] == [("direct", "direct-fenced", "canary")]
    assert any(key.endswith("_direct") for key in config["calibration_ms_per_apply"]) and line["transport_fallback"] is False
