"""``gt4py_amd.departure`` on the GPU: bit for bit against the contract's restatement (tests/departure_interp_ref.py), NaN compared
as NaN, over EVERY byte of each destination buffer -- row padding, ghost cells and the allocation's slack keep a NaN-payload
sentinel, compared as integers --, in the four layouts of tests/device_layouts.py, for float32 / float64 fields against float32 /
float64 positions, the four methods, absolute and relative positions, four reaches, IJ and IJK pos_i / pos_j, 1 to 9 fields per
call, at wave, workgroup and level-chunk boundaries and in every branch of the end-interval rule along K, with positions on
integers, halves, the ends of the readable box, beyond them, -0.0, +-inf, +-1e300 and NaN on all three axes, with an inf and a NaN
planted in the fields, against ``HorizontalInterp`` where no point leaves its level, and handed over from and to a stencil in
stream order."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import departure_interp_ref as D  # noqa: E402
import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

CHUNK_K = 8  # DEPARTURE_CHUNK_K of csrc/departure_interp.hip.h: the levels one thread walks
# nk = 1, 2, 3: every interval is an end interval; 4, 5: one / two intervals take the four-level formula; CHUNK_K + 1: two chunks
DOMAINS = [(1, 1, 1), (3, 2, 2), (5, 7, 3), (63, 4, 4), (64, 4, 5), (65, 5, 3), (130, 9, 4), (6, 3, CHUNK_K + 1)]
REACHES = [0, 1, 2, ((3, 1), (0, 2))]
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]  # (fields, positions)
COUNTS = [1, 4, 8, 9]


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_device_memory():
    """The few hundred small buffers of this file go back to the driver when it is done: what runs behind it in the same process
    (tests/test_placement.py searches the FREE device memory for a second memory group) finds no block of this file's in the
    caching allocator."""
    yield
    import torch

    torch.cuda.empty_cache()


def _reach4(reach):
    return (reach,) * 4 if isinstance(reach, int) else (reach[0][0], reach[0][1], reach[1][0], reach[1][1])


# ---- inputs: float64 arrays that hold values of the dtype the device gets, so that the restatement sees what the device sees ------
def _positions(rng, domain, reach4, pos3d, relative, pdtype):
    """(pos_i, pos_j, pos_k) over the domain -- pos_i / pos_j (ni, nj, nk) or (ni, nj), pos_k always (ni, nj, nk): random around the
    readable box with exact integers, exact halves, xmin and xmax themselves, points beyond both ends, -0.0, +-inf, +-1e300 and NaN
    planted at random points (as many as fit)."""
    ni, nj, nk = domain
    out = []
    for ax, (n, lo, hi) in enumerate(((ni, reach4[0], reach4[1]), (nj, reach4[2], reach4[3]), (nk, 0, 0))):
        shape = (ni, nj, nk) if pos3d or ax == 2 else (ni, nj)
        p = rng.uniform(-lo - 2.0, n + hi + 1.0, shape)
        kind = rng.integers(0, 5, shape)
        p = np.where(kind == 0, np.round(p), np.where(kind == 1, np.floor(p) + 0.5, p))
        special = np.array([-float(lo), float(n - 1 + hi), -lo - 1.5, n + hi + 0.25, -lo - 40.0, n + hi + 1000.0, -0.0, np.inf, -np.inf, 1e300,
                            -1e300, np.nan, 0.0, n - 1.0, -float(lo) + 0.5, n - 1 + hi - 0.5])
        where = rng.permutation(p.size)[: special.size]
        p.reshape(-1)[where] = special[rng.permutation(special.size)[: where.size]]
        if relative:
            p = p - np.arange(n, dtype=np.float64).reshape([-1 if ax == a else 1 for a in range(len(shape))])
        out.append(p)
    with np.errstate(over="ignore"):
        return [p.astype(pdtype) for p in out]


def _field_values(rng, shape, nfields, fdtype):
    out = []
    for n in range(nfields):
        if n % 3 == 0:
            q = rng.uniform(-1, 1, shape)
        elif n % 3 == 1:  # smooth and large: the cubic's overshoots are limited
            q = np.cumsum(np.cumsum(rng.uniform(0.1, 1, shape), axis=0), axis=1) * 10.0 ** rng.integers(-3, 4)
        else:
            q = 280.0 + rng.uniform(-1, 1, shape)
        out.append(q.astype(fdtype))
    return out


def _device_positions(positions, pos3d, shape, box, pdtype, layout, align, fill=7.25):
    """The three position fields on the device: (the Devs, what the product is given)."""
    devs, given = [], []
    for ax, p in enumerate(positions):
        full3d = pos3d or ax == 2
        pshape = shape if full3d else shape[:2] + (1,)
        full = np.full(pshape, fill, dtype=pdtype)
        full[box] = p if p.ndim == 3 else p[:, :, None]  # (2-d items in an IJK field: repeated along K)
        devs.append(L.Dev(pshape, pdtype, layout, full, align))
        given.append(devs[-1].given if full3d else devs[-1].given[:, :, 0])
    return devs, given


def _run(domain, method, *, fdtype=np.float64, pdtype=np.float64, layout="ifirst", reach=0, relative=False, pos3d=True, nfields=1, seed=0,
         order=None, plant=None, dst_layout=None, align=None):
    """One call through ``departure.DepartureInterp``; every dst buffer is compared whole against the restatement, every input must
    come back unchanged.  ``order``: which of the generated fields the call gets, in which order.  ``plant``: a list of ((i, j, k)
    in the readable box, value) set in every field.  Returns (the domain boxes as the device left them, by field number; the
    positions; the restatement's boxes)."""
    from gt4py_amd import departure

    ni, nj, nk = domain
    reach4 = _reach4(reach)
    lo_i, hi_i, lo_j, hi_j = reach4
    # (positions and fields from generators of their own: the same seed gives the same positions and the same first fields
    # whatever the layout, nfields or order is)
    rng_p, rng_q = (np.random.default_rng([seed, ni, nj, nk, lo_i, hi_i, lo_j, hi_j, what]) for what in (0, 1))
    # one ghost cell in front of the readable box on the low sides, one ghost row / column behind the array the product sees
    readable = (lo_i + ni + hi_i, lo_j + nj + hi_j)
    shape = (readable[0] + 2, readable[1] + 2, nk)
    origin = (1 + lo_i, 1 + lo_j, 0)
    box = (slice(origin[0], origin[0] + ni), slice(origin[1], origin[1] + nj))
    rbox = (slice(1, 1 + readable[0]), slice(1, 1 + readable[1]))
    positions = _positions(rng_p, domain, reach4, pos3d, relative, pdtype)
    order = list(range(nfields)) if order is None else list(order)
    qs = _field_values(rng_q, shape, max(order) + 1, fdtype)
    for at, value in plant or ():
        for q in qs:
            q[rbox][at] = value
    align = origin[0] if align is None else align
    d_pos, given_pos = _device_positions(positions, pos3d, shape, box, pdtype, layout, align)
    srcs = [L.Dev(shape, fdtype, layout, qs[n], align) for n in order]
    dsts = [L.Dev(shape, fdtype, dst_layout or layout, None, align) for _ in order]
    di = departure.DepartureInterp([d.given for d in dsts], [s.given for s in srcs], pos_i=given_pos[0], pos_j=given_pos[1], pos_k=given_pos[2],
                                   method=method, relative=relative, halo=reach, origin=origin)
    assert (di.domain, di.launches, di.method, di.relative, di.origin) == (domain, -(-len(order) // 8), method, relative, origin)
    di()
    what = (f"{method} {domain} {np.dtype(fdtype)} fields {np.dtype(pdtype)} positions {layout} reach {reach4} "
            f"{'relative' if relative else 'absolute'} {'IJK' if pos3d else 'IJ'} positions")
    got, want = {}, {}
    for slot, n in enumerate(order):
        want[n] = D.interp3(qs[n][rbox], *positions, method, relative, reach4)
        got[n] = dsts[slot].assert_box(box, want[n], f"{what}: dst {slot} (field {n}) of {len(order)}")
    for slot, s in enumerate(srcs):
        s.assert_unchanged(f"{what}: src {slot}")
    for name, d in zip(("pos_i", "pos_j", "pos_k"), d_pos):
        d.assert_unchanged(f"{what}: {name}")
    return got, positions, want


# ---- the grid: a seeded selection of the product that keeps every value of every factor ----------------------------------------------
FACTORS = (DOMAINS, L.LAYOUTS, DTYPES, list(D.METHODS), [False, True], REACHES, [False, True], COUNTS)


def _cases(count=64, seed=2027):
    rng = np.random.default_rng(seed)

    def column(values):
        reps = [values[n % len(values)] for n in range(count)]
        return [reps[n] for n in rng.permutation(count)]

    columns = [column(v) for v in FACTORS]
    for values, col in zip(FACTORS, columns):
        assert all(v in col for v in values)
    return list(zip(*columns))


def _case_id(case):
    domain, layout, (fd, pd), method, relative, reach, pos3d, count = case
    return (f"{'x'.join(map(str, domain))}-{layout}-{np.dtype(fd).name}-{np.dtype(pd).name}-{method}-{'rel' if relative else 'abs'}-"
            f"r{''.join(map(str, _reach4(reach)))}-{'ijk' if pos3d else 'ij'}-{count}")


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_every_byte_against_the_restatement(case):
    domain, layout, (fdtype, pdtype), method, relative, reach, pos3d, count = case
    _run(domain, method, fdtype=fdtype, pdtype=pdtype, layout=layout, reach=reach, relative=relative, pos3d=pos3d, nfields=count, seed=1)


@pytest.mark.parametrize("method", D.METHODS)
def test_every_special_position_is_among_the_inputs(method):
    """The largest domain holds every planted position on all three axes (the generator plants as many as fit), in both modes;
    along K the positions reach every branch of the end-interval rule."""
    for relative in (False, True):
        for pdtype in (np.float32, np.float64):
            _, positions, _ = _run((130, 9, 4), method, fdtype=np.float32, pdtype=pdtype, reach=((3, 1), (0, 2)), relative=relative, nfields=2,
                                   seed=2)
            for p, n, lo, hi, ax in zip(positions, (130, 9, 4), (3, 0, 0), (1, 2, 0), range(3)):
                x = p.astype(np.float64)
                if relative:
                    x = x + np.arange(n, dtype=np.float64).reshape([-1 if ax == a else 1 for a in range(3)])
                assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
                assert (x == -lo).any() and (x == n - 1 + hi).any() and (x < -lo).any() and (x > n - 1 + hi).any()
                finite = x[np.isfinite(x)]
                assert (finite == np.floor(finite)).any() and (finite - np.floor(finite) == 0.5).any()
                if not relative:
                    assert (np.signbit(p) & (p == 0)).any() and (x >= (1e300 if pdtype is np.float64 else np.inf)).any()
                    assert (x <= (-1e300 if pdtype is np.float64 else -np.inf)).any()
            b_k = np.floor(np.clip(x[~np.isnan(x)], 0, 3))  # (x: the K positions) nk = 4: b_k = 1 is the one four-level interval
            assert {0.0, 1.0, 2.0, 3.0} <= set(b_k.tolist())


@pytest.mark.parametrize("method", D.METHODS)
def test_a_planted_inf_and_nan_reach_exactly_the_points_whose_stencil_touches_them(method):
    domain, reach = (65, 5, 5), ((3, 1), (0, 2))
    reach4 = _reach4(reach)
    for fdtype in (np.float32, np.float64):
        kwargs = dict(fdtype=fdtype, reach=reach, nfields=2, seed=3, pos3d=True)
        clean, positions, clean_ref = _run(domain, method, **kwargs)
        planted = [((30, 3, 1), np.inf), ((0, 6, 2), np.nan), ((68, 0, 0), -np.inf), ((40, 2, 4), np.inf)]  # (one of them in a ghost cell)
        dirty, _, dirty_ref = _run(domain, method, plant=planted, **kwargs)
        mask = np.zeros((65 + 4, 5 + 2, 5), dtype=bool)
        for at, _ in planted:
            mask[at] = True
        nan_position = np.isnan(positions[0].astype(np.float64)) | np.isnan(positions[1].astype(np.float64)) | np.isnan(positions[2].astype(np.float64))
        touched = D.stencil_touches(mask, *positions, method, False, reach4) & ~nan_position
        assert touched.any() and not touched.all()
        for n in clean:
            differs = ~D.same_bits(clean[n], dirty[n])
            assert np.array_equal(differs, ~D.same_bits(clean_ref[n], dirty_ref[n]))  # as the restatement says
            assert not (differs & ~touched).any()  # no other point
            if method == D.CUBIC_MONOTONE:
                # an infinity outside the eight corners is limited away again: a point may come back to the clean value
                assert differs.any() and np.isnan(dirty[n][touched]).any()
            else:
                assert np.array_equal(differs, touched)  # a weight of zero still multiplies
            assert not np.isfinite(dirty[n][differs]).any() or method == D.CUBIC_MONOTONE


def test_the_bits_of_a_point_do_not_depend_on_layout_alignment_position_in_the_call_or_call_size():
    domain, reach = (65, 5, 5), 2
    for method in D.METHODS:
        kwargs = dict(fdtype=np.float32, pdtype=np.float64, reach=reach, relative=True, seed=4)
        nine, _, _ = _run(domain, method, nfields=9, **kwargs)  # two launches
        for layout in L.LAYOUTS[1:]:
            other, _, _ = _run(domain, method, nfields=4, layout=layout, **kwargs)
            for n in other:
                assert D.same_bits(other[n], nine[n]).all(), (method, layout, n)
        for align in (0, 1, 5):  # where in a 256-byte row the domain starts
            other, _, _ = _run(domain, method, nfields=1, align=align, dst_layout="kfirst", **kwargs)
            assert D.same_bits(other[0], nine[0]).all(), (method, align)
        # field 8 -- the second launch's first entry above -- alone, as entry 2 of 3, as the last of 8, and field 0 behind it
        for order in ([8], [3, 5, 8], [7, 6, 5, 4, 3, 2, 1, 8], [8, 0]):
            other, _, _ = _run(domain, method, order=order, **kwargs)
            for n in order:
                assert D.same_bits(other[n], nine[n]).all(), (method, order, n)


def test_a_field_of_ij_equals_an_ijk_field_with_the_same_items():
    """The same 2-d pos_i / pos_j once as Field[IJ] (computed once per chunk of levels) and once repeated along K (computed per
    level), over more levels than one chunk."""
    from gt4py_amd import departure

    ni, nj, nk, reach = 70, 6, CHUNK_K + 3, 1
    rng = np.random.default_rng(5)
    shape = (ni + 3, nj + 3, nk)  # one ghost cell on every side, one more row / column that the product does not see
    box = (slice(1, 1 + ni), slice(1, 1 + nj))
    for method in D.METHODS:
        for pdtype in (np.float32, np.float64):
            q = rng.uniform(-1, 1, shape).astype(np.float32)
            positions = _positions(rng, (ni, nj, nk), (1, 1, 1, 1), False, True, pdtype)
            src = L.Dev(shape, np.float32, "ifirst", q, 1)
            got = []
            for pos3d in (False, True):
                _, given = _device_positions(positions, pos3d, shape, box, pdtype, "ifirst", 1, fill=0.0)
                dst = L.Dev(shape, np.float32, "ifirst", None, 1)
                departure.interpolate_3d(dst.given, src.given, pos_i=given[0], pos_j=given[1], pos_k=given[2], method=method, relative=True,
                                         halo=reach)
                want = D.interp3(q[:-1, :-1], *positions, method, True, (1, 1, 1, 1))
                got.append(dst.assert_box(box, want, f"{method} {'IJK' if pos3d else 'IJ'} positions"))
            assert D.same_bits(got[0], got[1]).all()


@pytest.mark.parametrize("method", ["nearest", "linear", "cubic"])
def test_with_every_point_on_its_own_level_the_device_result_is_that_of_horizontal_interp(method):
    """pos_k holds each point's own level (absolute) or 0 (relative): DepartureInterp's bytes are HorizontalInterp's, on fields of
    280 +- 1 (finite non-zero plane values: the K weights (1, 0) and (-0, 1, 0, -0) reproduce them)."""
    from gt4py_amd import departure, horizontal

    reach = 2
    rng = np.random.default_rng(7)
    for (ni, nj, nk), fdtype, relative in (((65, 5, 3), np.float32, False), ((33, 6, CHUNK_K + 2), np.float64, True), ((7, 3, 1), np.float64, False)):
        shape = (ni + 2 * reach + 1, nj + 2 * reach + 1, nk)
        box = (slice(reach, reach + ni), slice(reach, reach + nj))
        q = (280.0 + rng.uniform(-1, 1, shape)).astype(fdtype)
        pi, pj, _ = _positions(rng, (ni, nj, nk), (reach,) * 4, True, relative, np.float64)
        # (no NaN position here: which NaN an operation on a NaN yields is not part of the contract -- payloads are compared nowhere --,
        # and this test compares BYTES; NaN positions are held against the restatement in the tests above)
        pi, pj = np.where(np.isnan(pi), 0.25, pi), np.where(np.isnan(pj), -0.75, pj)
        pk = np.zeros((ni, nj, nk)) if relative else np.broadcast_to(np.arange(nk, dtype=np.float64), (ni, nj, nk))
        _, given = _device_positions((pi, pj, pk), True, shape, box, np.float64, "ifirst", reach)
        src = L.Dev(shape, fdtype, "ifirst", q, reach)
        want = D.interp3(q[:-1, :-1], pi, pj, pk, method, relative, (reach,) * 4)
        ours, theirs = L.Dev(shape, fdtype, "ifirst", None, reach), L.Dev(shape, fdtype, "ifirst", None, reach)
        departure.interpolate_3d(ours.given, src.given, pos_i=given[0], pos_j=given[1], pos_k=given[2], method=method, relative=relative, halo=reach)
        horizontal.interpolate(theirs.given, src.given, pos_i=given[0], pos_j=given[1], method=method, relative=relative, halo=reach)
        # (each against the restatement over its whole buffer, then against each other byte for byte)
        a = ours.assert_box(box, want, f"{method} {(ni, nj, nk)}: DepartureInterp")
        b = theirs.assert_box(box, want, f"{method} {(ni, nj, nk)}: HorizontalInterp")
        assert np.array_equal(a.view(L.NP_UINT[a.itemsize]), b.view(L.NP_UINT[b.itemsize]))


def test_hand_over_from_a_stencil_and_to_a_stencil_in_stream_order():
    """A device_sync=False stencil writes the three displacement fields, DepartureInterp gathers, a device_sync=False stencil reads
    the result, nothing in between: the stencils applied to the restatement."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import departure
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    def displacements(u: gtscript.Field[np.float64], v: gtscript.Field[np.float64], w: gtscript.Field[np.float64],
                      di: gtscript.Field[np.float64], dj: gtscript.Field[np.float64], dk: gtscript.Field[np.float64], *, cx: float, cy: float,
                      cz: float):
        with computation(PARALLEL), interval(...):  # noqa: F821
            di = -u * cx  # noqa: F841
            dj = -v * cy  # noqa: F841
            dk = -w * cz  # noqa: F841

    backend, (ni, nj, nk), h = "hip:mi300", (96, 40, 9), 3
    rng = np.random.default_rng(6)
    shape = (ni + 2 * h, nj + 2 * h, nk)
    q, u, v, w = (rng.uniform(-1, 1, shape) for _ in range(4))
    cx, cy, cz = 2.75, 1.5, 1.75  # |displacement| < 3 = the halo along I and J; K is clamped to the levels
    disp = gtscript.stencil(backend=backend, definition=displacements, device_sync=False)
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_q, d_u, d_v, d_w = (gt_storage.from_array(a, backend=backend, aligned_index=(h, h, 0)) for a in (q, u, v, w))
    d_di, d_dj, d_dk, d_new, d_out = (gt_storage.zeros(shape, backend=backend, aligned_index=(h, h, 0)) for _ in range(5))
    advect = departure.DepartureInterp([d_new], [d_q], pos_i=d_di, pos_j=d_dj, pos_k=d_dk, relative=True, method="cubic_monotone", halo=h)
    assert advect.domain == (ni, nj, nk) and advect.origin == (h, h, 0)
    for _ in range(2):  # (the second round finds everything already written: the same result)
        disp(d_u, d_v, d_w, d_di, d_dj, d_dk, cx=cx, cy=cy, cz=cz, origin=(h, h, 0), domain=(ni, nj, nk))
        advect()
        lap(d_new, d_out, origin=(h + 1, h + 1, 0), domain=(ni - 2, nj - 2, nk))
    torch.cuda.synchronize()
    box = (slice(h, h + ni), slice(h, h + nj))
    di, dj, dk = -u[box] * cx, -v[box] * cy, -w[box] * cz
    new = np.zeros(shape)
    new[box] = D.interp3(q, di, dj, dk, D.CUBIC_MONOTONE, True, (h, h, h, h))
    want = np.zeros(shape)
    ORACLE.laplacian(new, want, origin_inp=(h + 1, h + 1, 0), origin_out=(h + 1, h + 1, 0), domain=(ni - 2, nj - 2, nk))
    assert np.array_equal(d_dk.get()[box].view(np.uint64), dk.view(np.uint64))
    assert np.array_equal(d_new.get().view(np.uint64), new.view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))


def test_the_c_entry_counts_what_it_enqueued():
    import torch

    from gt4py_amd import _lib, departure

    shape = (9, 4, 3)
    rng = np.random.default_rng(9)
    srcs = [L.Dev(shape, np.float64, "ifirst", q) for q in _field_values(rng, shape, 9, np.float64)]
    dsts = [L.Dev(shape, np.float64, "ifirst", None) for _ in srcs]
    pos = L.Dev(shape, np.float64, "ifirst", rng.uniform(0, 3, shape))
    di = departure.DepartureInterp([d.given for d in dsts], [s.given for s in srcs], pos_i=pos.given, pos_j=pos.given, pos_k=pos.given)
    launches = ctypes.c_int(-1)
    rc = _lib.load().gt4mi_departure_interp(di._dst, di._src, 9, ctypes.byref(di._pos_i), ctypes.byref(di._pos_j), ctypes.byref(di._pos_k),
                                            di._extent, di._reach, 8, 8, _lib.INTERP_LINEAR, 0, torch.cuda.current_stream().cuda_stream,
                                            ctypes.byref(launches))
    torch.cuda.synchronize()
    assert rc == 0 and launches.value == 2
