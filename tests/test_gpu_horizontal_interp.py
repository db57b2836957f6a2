"""``gt4py_amd.horizontal`` on the GPU: bit for bit against the contract's restatement (tests/horizontal_interp_ref.py), NaN
compared as NaN, over EVERY byte of each destination buffer -- row padding, ghost cells and the allocation's slack keep a
NaN-payload sentinel, compared as integers --, in the four layouts of tests/device_layouts.py, for float32 / float64 fields against
float32 / float64 positions, the four methods, absolute and relative positions, four reaches, IJ and IJK position fields, 1 to 9
fields per call, at wave, workgroup and level-chunk boundaries, with positions on integers, halves, the ends of the readable box,
beyond them, -0.0, +-inf, 1e300 and NaN, with an inf and a NaN planted in the fields, and handed over from and to a stencil in
stream order."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import horizontal_interp_ref as H  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

CHUNK_K = 8  # INTERP_CHUNK_K of csrc/horizontal_interp.hip.h: the levels one thread walks
DOMAINS = [(1, 1, 1), (3, 2, 1), (5, 7, 3), (63, 4, 2), (64, 4, 2), (65, 5, 3), (130, 9, 4), (6, 3, CHUNK_K + 1)]
REACHES = [0, 1, 2, ((3, 1), (0, 2))]
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]  # (fields, positions)
COUNTS = [1, 4, 8, 9]


def _reach4(reach):
    return (reach,) * 4 if isinstance(reach, int) else (reach[0][0], reach[0][1], reach[1][0], reach[1][1])


# ---- inputs: float64 arrays that hold values of the dtype the device gets, so that the restatement sees what the device sees ------
def _positions(rng, domain, reach4, pos3d, relative, pdtype):
    """(pos_i, pos_j) over the domain, (ni, nj, nk) or (ni, nj): random around the readable box with exact integers, exact halves,
    xmin and xmax themselves, points beyond both ends, -0.0, +-inf, 1e300 and NaN planted at random points (as many as fit)."""
    ni, nj, nk = domain
    shape = (ni, nj, nk) if pos3d else (ni, nj)
    out = []
    for n, lo, hi in ((ni, reach4[0], reach4[1]), (nj, reach4[2], reach4[3])):
        p = rng.uniform(-lo - 2.0, n + hi + 1.0, shape)
        kind = rng.integers(0, 5, shape)
        p = np.where(kind == 0, np.round(p), np.where(kind == 1, np.floor(p) + 0.5, p))
        special = np.array([-float(lo), float(n - 1 + hi), -lo - 1.5, n + hi + 0.25, -lo - 40.0, n + hi + 1000.0, -0.0, np.inf, -np.inf, 1e300,
                            -1e300, np.nan, 0.0, n - 1.0, -float(lo) + 0.5, n - 1 + hi - 0.5])
        where = rng.permutation(p.size)[: special.size]
        p.reshape(-1)[where] = special[rng.permutation(special.size)[: where.size]]
        out.append(p)
    if relative:
        index = [np.arange(n, dtype=np.float64).reshape([-1 if ax == a else 1 for a in range(len(shape))]) for ax, n in enumerate((ni, nj))]
        out = [p - x for p, x in zip(out, index)]
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


def _run(domain, method, *, fdtype=np.float64, pdtype=np.float64, layout="ifirst", reach=0, relative=False, pos3d=True, nfields=1, seed=0,
         order=None, plant=None, dst_layout=None, align=None):
    """One call through ``horizontal.HorizontalInterp``; every dst buffer is compared whole against the restatement, every input
    must come back unchanged.  ``order``: which of the generated fields the call gets, in which order.  ``plant``: a list of
    ((i, j, k) in the readable box, value) set in every field.  Returns (the domain boxes as the device left them, by field number;
    the positions; the restatement's boxes)."""
    from gt4py_amd import horizontal

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
    pi, pj = _positions(rng_p, domain, reach4, pos3d, relative, pdtype)
    order = list(range(nfields)) if order is None else list(order)
    qs = _field_values(rng_q, shape, max(order) + 1, fdtype)
    for at, value in plant or ():
        for q in qs:
            q[rbox][at] = value
    align = origin[0] if align is None else align
    pshape = shape if pos3d else shape[:2] + (1,)
    d_pos = []
    for p in (pi, pj):
        full = np.full(pshape, 7.25, dtype=pdtype)
        full[box] = p if pos3d else p[:, :, None]
        d_pos.append(L.Dev(pshape, pdtype, layout, full, align))
    given_pos = [d.given if pos3d else d.given[:, :, 0] for d in d_pos]
    srcs = [L.Dev(shape, fdtype, layout, qs[n], align) for n in order]
    dsts = [L.Dev(shape, fdtype, dst_layout or layout, None, align) for _ in order]
    hi = horizontal.HorizontalInterp([d.given for d in dsts], [s.given for s in srcs], pos_i=given_pos[0], pos_j=given_pos[1], method=method,
                                     relative=relative, halo=reach, origin=origin)
    assert (hi.domain, hi.launches, hi.method) == (domain, -(-len(order) // 8), method)
    hi()
    what = (f"{method} {domain} {np.dtype(fdtype)} fields {np.dtype(pdtype)} positions {layout} reach {reach4} "
            f"{'relative' if relative else 'absolute'} {'IJK' if pos3d else 'IJ'} positions")
    got, want = {}, {}
    for slot, n in enumerate(order):
        want[n] = H.interp(qs[n][rbox], pi, pj, method, relative, reach4)
        got[n] = dsts[slot].assert_box(box, want[n], f"{what}: dst {slot} (field {n}) of {len(order)}")
    for slot, s in enumerate(srcs):
        s.assert_unchanged(f"{what}: src {slot}")
    for name, d in zip(("pos_i", "pos_j"), d_pos):
        d.assert_unchanged(f"{what}: {name}")
    return got, (pi, pj), want


# ---- the grid: a seeded selection of the product that keeps every value of every factor ----------------------------------------------
def _cases(count=64, seed=2026):
    rng = np.random.default_rng(seed)

    def column(values):
        reps = [values[n % len(values)] for n in range(count)]
        return [reps[n] for n in rng.permutation(count)]

    columns = [column(v) for v in (DOMAINS, L.LAYOUTS, DTYPES, list(H.METHODS), [False, True], REACHES, [False, True], COUNTS)]
    cases = list(zip(*columns))
    for values, col in zip((DOMAINS, L.LAYOUTS, DTYPES, list(H.METHODS), [False, True], REACHES, [False, True], COUNTS), columns):
        assert all(v in col for v in values)
    return cases


def _case_id(case):
    domain, layout, (fd, pd), method, relative, reach, pos3d, count = case
    return (f"{'x'.join(map(str, domain))}-{layout}-{np.dtype(fd).name}-{np.dtype(pd).name}-{method}-{'rel' if relative else 'abs'}-"
            f"r{''.join(map(str, _reach4(reach)))}-{'ijk' if pos3d else 'ij'}-{count}")


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_every_byte_against_the_restatement(case):
    domain, layout, (fdtype, pdtype), method, relative, reach, pos3d, count = case
    _run(domain, method, fdtype=fdtype, pdtype=pdtype, layout=layout, reach=reach, relative=relative, pos3d=pos3d, nfields=count, seed=1)


@pytest.mark.parametrize("method", H.METHODS)
def test_every_special_position_is_among_the_inputs(method):
    """The largest domain holds every planted position on both axes (the generator plants as many as fit), in both modes."""
    for relative in (False, True):
        for pdtype in (np.float32, np.float64):
            _, (pi, pj), _ = _run((130, 9, 4), method, fdtype=np.float32, pdtype=pdtype, reach=((3, 1), (0, 2)), relative=relative, nfields=2, seed=2)
            for p, n, lo, hi, ax in ((pi, 130, 3, 1, 0), (pj, 9, 0, 2, 1)):
                x = p.astype(np.float64)
                if relative:
                    x = x + np.arange(n, dtype=np.float64).reshape([-1 if ax == a else 1 for a in range(3)])
                assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
                assert (x == -lo).any() and (x == n - 1 + hi).any() and (x < -lo).any() and (x > n - 1 + hi).any()
                finite = x[np.isfinite(x)]
                assert (finite == np.floor(finite)).any() and (finite - np.floor(finite) == 0.5).any()
                if not relative:
                    assert (np.signbit(p) & (p == 0)).any() and (x >= (1e300 if pdtype is np.float64 else np.inf)).any()


@pytest.mark.parametrize("method", H.METHODS)
def test_a_planted_inf_and_nan_reach_exactly_the_points_whose_stencil_touches_them(method):
    domain, reach = (65, 5, 3), ((3, 1), (0, 2))
    reach4 = _reach4(reach)
    for fdtype in (np.float32, np.float64):
        kwargs = dict(fdtype=fdtype, reach=reach, nfields=2, seed=3, pos3d=True)
        clean, (pi, pj), clean_ref = _run(domain, method, **kwargs)
        planted = [((30, 3, 1), np.inf), ((0, 6, 2), np.nan), ((68, 0, 0), -np.inf)]  # (in the readable box: one of them in a ghost cell)
        dirty, _, dirty_ref = _run(domain, method, plant=planted, **kwargs)
        mask = np.zeros((65 + 4, 5 + 2, 3), dtype=bool)
        for at, _ in planted:
            mask[at] = True
        nan_position = np.isnan(pi.astype(np.float64)) | np.isnan(pj.astype(np.float64))
        touched = H.stencil_touches(mask, pi, pj, method, False, reach4) & ~nan_position
        assert touched.any() and not touched.all()
        for n in clean:
            differs = ~H.same_bits(clean[n], dirty[n])
            assert np.array_equal(differs, ~H.same_bits(clean_ref[n], dirty_ref[n]))  # as the restatement says
            assert not (differs & ~touched).any()  # no other point
            if method == H.CUBIC_MONOTONE:
                # an infinity outside the four corners is limited away again: a point may come back to the clean value
                assert differs.any() and np.isnan(dirty[n][touched]).any()
            else:
                assert np.array_equal(differs, touched)  # a weight of zero still multiplies
            assert not np.isfinite(dirty[n][differs]).any() or method == H.CUBIC_MONOTONE


def test_the_bits_of_a_point_do_not_depend_on_layout_alignment_position_in_the_call_or_call_size():
    domain, reach = (65, 5, 3), 2
    for method in H.METHODS:
        kwargs = dict(fdtype=np.float32, pdtype=np.float64, reach=reach, relative=True, seed=4)
        nine, _, _ = _run(domain, method, nfields=9, **kwargs)  # two launches
        for layout in L.LAYOUTS[1:]:
            other, _, _ = _run(domain, method, nfields=4, layout=layout, **kwargs)
            for n in other:
                assert H.same_bits(other[n], nine[n]).all(), (method, layout, n)
        for align in (0, 1, 5):  # where in a 256-byte row the domain starts
            other, _, _ = _run(domain, method, nfields=1, align=align, dst_layout="kfirst", **kwargs)
            assert H.same_bits(other[0], nine[0]).all(), (method, align)
        # field 8 -- the second launch's first entry above -- alone, as entry 2 of 3, as the last of 8, and field 0 behind it
        for order in ([8], [3, 5, 8], [7, 6, 5, 4, 3, 2, 1, 8], [8, 0]):
            other, _, _ = _run(domain, method, order=order, **kwargs)
            for n in order:
                assert H.same_bits(other[n], nine[n]).all(), (method, order, n)


def test_a_field_of_ij_equals_an_ijk_field_with_the_same_items():
    """The same 2-d positions once as a Field[IJ] (computed once per chunk of levels) and once repeated along K (computed per
    level), over more levels than one chunk."""
    from gt4py_amd import horizontal

    ni, nj, nk, reach = 70, 6, CHUNK_K + 3, 1
    rng = np.random.default_rng(5)
    shape = (ni + 3, nj + 3, nk)  # one ghost cell on every side, one more row / column that the product does not see
    for method in H.METHODS:
        for pdtype in (np.float32, np.float64):
            q = rng.uniform(-1, 1, shape).astype(np.float32)
            pi, pj = _positions(rng, (ni, nj, nk), (1, 1, 1, 1), False, True, pdtype)
            src = L.Dev(shape, np.float32, "ifirst", q, 1)
            got = []
            for pos3d in (False, True):
                pshape = shape if pos3d else shape[:2] + (1,)
                d_pos = []
                for p in (pi, pj):
                    full = np.zeros(pshape, dtype=pdtype)
                    full[1:1 + ni, 1:1 + nj] = p[:, :, None]
                    d_pos.append(L.Dev(pshape, pdtype, "ifirst", full, 1))
                given = [d.given if pos3d else d.given[:, :, 0] for d in d_pos]
                dst = L.Dev(shape, np.float32, "ifirst", None, 1)
                horizontal.interpolate(dst.given, src.given, pos_i=given[0], pos_j=given[1], method=method, relative=True, halo=reach)
                want = H.interp(q[:-1, :-1], pi, pj, method, True, (1, 1, 1, 1))
                got.append(dst.assert_box((slice(1, 1 + ni), slice(1, 1 + nj)), want, f"{method} {'IJK' if pos3d else 'IJ'} positions"))
            assert H.same_bits(got[0], got[1]).all()


def test_hand_over_from_a_stencil_and_to_a_stencil_in_stream_order():
    """A device_sync=False stencil writes the displacements, HorizontalInterp gathers, a device_sync=False stencil reads the result,
    nothing in between: the stencils applied to the restatement."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import horizontal
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    def displacements(u: gtscript.Field[np.float64], v: gtscript.Field[np.float64], di: gtscript.Field[np.float64],
                      dj: gtscript.Field[np.float64], *, cx: float, cy: float):
        with computation(PARALLEL), interval(...):  # noqa: F821
            di = -u * cx  # noqa: F841
            dj = -v * cy  # noqa: F841

    backend, (ni, nj, nk), h = "hip:mi300", (96, 40, 5), 3
    rng = np.random.default_rng(6)
    shape = (ni + 2 * h, nj + 2 * h, nk)
    q, u, v = (rng.uniform(-1, 1, shape) for _ in range(3))
    cx, cy = 2.75, 1.5  # |displacement| < 3 = the halo
    disp = gtscript.stencil(backend=backend, definition=displacements, device_sync=False)
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_q, d_u, d_v = (gt_storage.from_array(a, backend=backend, aligned_index=(h, h, 0)) for a in (q, u, v))
    d_di, d_dj, d_new, d_out = (gt_storage.zeros(shape, backend=backend, aligned_index=(h, h, 0)) for _ in range(4))
    advect = horizontal.HorizontalInterp([d_new], [d_q], pos_i=d_di, pos_j=d_dj, relative=True, method="cubic_monotone", halo=h)
    assert advect.domain == (ni, nj, nk) and advect.origin == (h, h, 0)
    for _ in range(2):  # (the second round finds everything already written: the same result)
        disp(d_u, d_v, d_di, d_dj, cx=cx, cy=cy, origin=(h, h, 0), domain=(ni, nj, nk))
        advect()
        lap(d_new, d_out, origin=(h + 1, h + 1, 0), domain=(ni - 2, nj - 2, nk))
    torch.cuda.synchronize()
    box = (slice(h, h + ni), slice(h, h + nj))
    di, dj = -u[box] * cx, -v[box] * cy
    new = np.zeros(shape)
    new[box] = H.interp(q, di, dj, H.CUBIC_MONOTONE, True, (h, h, h, h))
    want = np.zeros(shape)
    ORACLE.laplacian(new, want, origin_inp=(h + 1, h + 1, 0), origin_out=(h + 1, h + 1, 0), domain=(ni - 2, nj - 2, nk))
    assert np.array_equal(d_di.get()[box].view(np.uint64), di.view(np.uint64))
    assert np.array_equal(d_new.get().view(np.uint64), new.view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))


def test_the_c_entry_counts_what_it_enqueued():
    import torch

    from gt4py_amd import _lib, horizontal

    shape = (9, 4, 2)
    rng = np.random.default_rng(9)
    srcs = [L.Dev(shape, np.float64, "ifirst", q) for q in _field_values(rng, shape, 9, np.float64)]
    dsts = [L.Dev(shape, np.float64, "ifirst", None) for _ in srcs]
    pos = L.Dev(shape, np.float64, "ifirst", rng.uniform(0, 3, shape))
    hi = horizontal.HorizontalInterp([d.given for d in dsts], [s.given for s in srcs], pos_i=pos.given, pos_j=pos.given)
    launches = ctypes.c_int(-1)
    rc = _lib.load().gt4mi_horizontal_interp(hi._dst, hi._src, 9, ctypes.byref(hi._pos_i), ctypes.byref(hi._pos_j), hi._extent, hi._reach, 8, 8,
                                             _lib.INTERP_LINEAR, 0, torch.cuda.current_stream().cuda_stream, ctypes.byref(launches))
    torch.cuda.synchronize()
    assert rc == 0 and launches.value == 2
