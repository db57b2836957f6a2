"""tests/stencil_geometries.py itself, and what tests/test_gpu_fuzz_geometries.py covers with it -- all without a device: every
geometry delivers what its one-liner claims, the numpy oracle does not care about geometry, the comparison routine catches a
single planted item in every kind of place, and a census of the twins `hip_generic.select_twin` names over the GPU file's seeds."""

import collections
import types

import numpy as np
import pytest

import stencil_geometries as G
import test_gpu_fuzz_geometries as T

DTYPES = {1: np.int8, 2: np.int16, 4: np.float32, 8: np.float64}


def _toy(itemsize, domain=(37, 11, 3), geometry="preset"):
    """Three I-J-K fields with different halos (`out` written), one K field kept plain; host buffers at their real addresses."""
    dt = np.dtype(DTYPES[itemsize])
    rng = np.random.default_rng(3)
    info = {k: types.SimpleNamespace(axes=("I", "J", "K"), data_dims=()) for k in ("a", "b", "out")}
    info["prof"] = types.SimpleNamespace(axes=("K",), data_dims=())
    origins = {"a": (2, 1, 0), "b": (3, 3, 1), "out": (0, 0, 0), "prof": (0,)}
    halo_hi = {"a": (2, 1, 0), "b": (0, 2, 1), "out": (0, 0, 0)}
    arrays = {k: rng.integers(1, 100, tuple(d + lo + hi for d, lo, hi in zip(domain, origins[k], halo_hi[k]))).astype(dt) for k in halo_hi}
    arrays["prof"] = rng.integers(1, 100, (domain[2],)).astype(dt)
    case = G.Case(geometry, arrays, origins, info, {"out"}, domain)
    images = {buf: G.L.sentinel_image(numel, isz) for buf, (numel, isz) in case.buffers.items()}
    ptr_of = {buf: image.ctypes.data for buf, image in images.items()}
    case.resolve(ptr_of)
    return case, arrays, ptr_of


@pytest.mark.parametrize("itemsize", [1, 2, 4, 8])
@pytest.mark.parametrize("geometry", list(G.GEOMETRIES))
def test_every_geometry_delivers_what_it_claims(geometry, itemsize):
    from gt4py_amd.cartesian.backend.hip_generic import elements_disjoint

    case, arrays, ptr_of = _toy(itemsize, geometry=geometry)
    lane = G.lane(itemsize)
    assert set(case.fields) == {"a", "b", "out"} and set(case.plain) == {"prof"}
    org = {k: case.origin_pointer(ptr_of, k) % 16 for k in case.fields}
    si, sj, sk = ({k: case.fields[k][2][n] for k in case.fields} for n in range(3))
    spans = sorted(case.span(ptr_of, k) for k in case.fields)
    overlap = any(spans[n][1] > spans[n + 1][0] for n in range(2))
    shifted = {"lead1": 1, "lead2": 2, "lead3": 3, "sub_box": 5}.get(geometry, 0)
    if geometry in ("preset", "lead1", "lead2", "lead3", "sub_box", "mixed_lead", "odd_plane", "j_halves"):
        for k in case.fields:
            off = 1 if k == case.off_column else shifted
            off += case.origins[k][2] if geometry == "odd_plane" else 0  # (a K origin of n: n odd planes further on)
            assert org[k] == (off * itemsize) % 16 and si[k] == 1 and sj[k] % lane == 0, (k, org, sj)
            assert (sk[k] % lane == 0) != (geometry == "odd_plane" and lane > 1)
    if geometry == "mixed_lead":
        assert case.off_column == "out"
    if geometry == "odd_pitch":
        assert all(si[k] == 1 and sj[k] % 2 == 1 and (lane == 1 or sj[k] % lane) for k in case.fields)
    if geometry in ("kfirst", "jfirst"):
        assert all(si[k] > 1 for k in case.fields) and {k: (sj[k], sk[k]) for k in case.fields} == {
            k: ((s[2], 1) if geometry == "kfirst" else (1, (s[0] + 1) * (s[1] + 1))) for k, s in case.shape.items() if k in case.fields}
    if geometry == "sub_box":
        assert case.domain == (31, 8, 3) and case.origins == {"a": (7, 3, 0), "b": (8, 5, 1), "out": (5, 2, 0), "prof": (0,)}
    else:
        assert case.domain == (37, 11, 3)
    assert overlap == (geometry in G.ALIAS)
    if geometry in G.ALIAS:
        a, b = case.pair
        assert (a, b) == ("out", "a") and case.fields[a][0] == case.fields[b][0] and case.fields[a][2] == case.fields[b][2]
        assert si[a] == (1 if geometry == "j_halves" else 2)
        byte_strides = tuple(s * itemsize for s in case.fields[a][2])
        assert elements_disjoint(case.span(ptr_of, a)[0], case.shape[a], case.span(ptr_of, b)[0], case.shape[b], byte_strides, itemsize)
        cells = [set((case.span(ptr_of, k)[0] + np.indices(case.shape[k]).reshape(3, -1).T @ np.array(byte_strides)).tolist()) for k in (a, b)]
        assert not cells[0] & cells[1]  # (and by enumeration)
    assert G.VARIANT[geometry] == (all(s == 1 for s in si.values()), not overlap)
    # the views do not leave their buffers, ghosts included, and no two rows share an item
    for k, (buf, shape, strides) in case.fields.items():
        ext = case._ext(k)
        index = case.offset[k] + np.indices(ext).reshape(3, -1).T @ np.array(strides)
        assert index.min() >= 0 and index.max() < case.buffers[buf][0] and np.unique(index).size == index.size


def test_alias_geometries_are_left_out_only_for_want_of_a_pair():
    info = {k: types.SimpleNamespace(axes=("I", "J", "K"), data_dims=()) for k in ("a", "out")}
    arrays = {"a": np.zeros((5, 4, 3), np.float32), "out": np.zeros((5, 4, 3), np.float64)}
    for geometry in G.ALIAS:
        with pytest.raises(G.LeftOut, match="no two I-J-K fields of equal item size"):
            G.Case(geometry, arrays, {"a": (0, 0, 0), "out": (0, 0, 0)}, info, {"out"}, (5, 4, 3))


# ---- the oracle on strided views ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, seed", [("structural", s) for s in range(12)] + [("typed", s) for s in range(12)])
def test_the_oracle_gives_the_same_bits_on_the_strided_views_of_every_geometry(kind, seed, tmp_path):
    from test_oracle_independent import assert_same_bits, defined_casts_only

    ref, hip, scalars, text = T.build(kind, seed, tmp_path)
    oracle = {}
    for geometry, domain, arrays, origins, case in T.cases(kind, seed, ref, hip, text):
        if isinstance(case, G.LeftOut):
            continue
        expect = oracle.setdefault(domain, T.Oracle(kind, ref, scalars))(case, arrays)
        images = {buf: G.L.sentinel_image(numel, isz) for buf, (numel, isz) in case.buffers.items()}
        case.resolve({buf: image.ctypes.data for buf, image in images.items()})
        before = case.images(arrays)
        for buf in images:
            images[buf][...] = before[buf]
        views = case.host_views(images)
        plain = {k: arrays[k].copy() for k in case.plain}
        with defined_casts_only():
            ref(**views, **plain, **scalars, origin=case.origins, domain=case.domain)
        what = f"{kind} seed {seed}, geometry {geometry}, domain {case.domain}"
        for k in arrays:
            assert_same_bits(np.ascontiguousarray(views[k]) if k in views else plain[k], expect[k], f"{what}: field {k}\n{text}")
        case.compare(before, expect, images, what)  # ... and nothing outside the views


# ---- the comparison routine: one planted item per kind of place -----------------------------------------------------------------
ODD_BITS = 0  # fits every item size; no value (1..100), sentinel or NaN of these tests


def _compared(geometry="preset", itemsize=8):
    """(case, before, expect, got): a call that wrote `expect["out"]` and nothing else."""
    case, arrays, _ = _toy(itemsize, geometry=geometry)
    before = case.images(arrays)
    expect = {k: v.copy() for k, v in arrays.items()}
    expect["out"] = (expect["out"] + 1).astype(expect["out"].dtype)
    got = {buf: image.copy() for buf, image in before.items()}
    case.view(got, "out")[...] = expect["out"].view(G.L.NP_INT[itemsize])
    return case, before, expect, got


def _places(case, k):
    buf, shape, strides = case.fields[k]
    covered = np.zeros(case.buffers[buf][0], dtype=bool)
    for other in case.fields:
        if case.fields[other][0] == buf:
            G.L.host_view(covered, case._ext(other), case.fields[other][2], case.offset[other])[...] = True
    free = np.flatnonzero(~covered)
    last = int(np.flatnonzero(covered)[-1])
    places = {"inside": case.offset[k] + sum(strides), "ghost cell": case.offset[k] + shape[0] * strides[0]}
    if strides[0] < strides[1] < strides[2]:  # padded rows
        places.update({"row padding": int(free[(free > case.offset[k]) & (free < last)][0]), "slack": int(free[free > last][-1])})
    return places


@pytest.mark.parametrize("geometry", ["preset", "lead3", "odd_plane", "j_halves", "interleaved"])
@pytest.mark.parametrize("itemsize", [1, 8])
def test_the_comparison_passes_when_only_the_written_view_changed(geometry, itemsize):
    case, before, expect, got = _compared(geometry, itemsize)
    case.compare(before, expect, got, "case")


@pytest.mark.parametrize("geometry", ["preset", "j_halves", "interleaved"])
@pytest.mark.parametrize("place, in_view", [("inside", 1), ("ghost cell", 0), ("row padding", 0), ("slack", 0)])
def test_one_planted_item_is_caught(geometry, place, in_view):
    case, before, expect, got = _compared(geometry)
    index = _places(case, "out")[place]
    got[case.fields["out"][0]][index] = ODD_BITS
    with pytest.raises(AssertionError, match=rf"case: buffer of .*out.*: 1 items of the whole buffer differ \({in_view} of them in a view\), "
                                             rf"first at flat index \[{index}\]"):
        case.compare(before, expect, got, "case")


@pytest.mark.parametrize("geometry", ["preset", "kfirst", "j_halves"])
def test_one_planted_item_in_an_untouched_input_is_caught(geometry):
    case, before, expect, got = _compared(geometry)
    index = _places(case, "b")["inside"]
    got[case.fields["b"][0]][index] = ODD_BITS
    with pytest.raises(AssertionError, match=rf"1 items of the whole buffer differ \(1 of them in a view\), first at flat index \[{index}\]"):
        case.compare(before, expect, got, "case")


def test_nan_payloads_and_the_sign_of_zero():
    """Inside a written view a NaN matches a NaN of any payload; -0.0 against 0.0 does not; in an input, NaN payloads count."""
    case, before, expect, got = _compared()
    expect["out"][1, 1, 1] = np.nan
    case.view(got, "out")[1, 1, 1] = 0x7FF8_0000_0BAD_F00D
    case.compare(before, expect, got, "case")
    expect["out"][2, 1, 1] = 0.0
    case.view(got, "out")[2, 1, 1] = np.array(-0.0).view(np.int64)
    with pytest.raises(AssertionError, match="1 items of the whole buffer differ"):
        case.compare(before, expect, got, "case")
    case, before, expect, got = _compared()
    case.view(got, "b")[1, 1, 1] = 0x7FF8_0000_0BAD_F00D
    with pytest.raises(AssertionError, match="1 items of the whole buffer differ"):
        case.compare(before, expect, got, "case")


# ---- census and cap, over the seeds of the GPU file -----------------------------------------------------------------------------
LANE_TWINS = ("vec", "vecs")


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    """[(kind, seed, geometry, domain, variant key, lead, [(kernel record, label)])] and the cases left out, {(kind, geometry): n}."""
    tmp = tmp_path_factory.mktemp("census")
    rows, left, total = [], collections.Counter(), collections.Counter()
    seeds = [("structural", s) for s in T.STRUCTURAL_SEEDS] + [("typed", s) for s in T.TYPED_SEEDS]
    seeds += [ks for ks in T.NAMED_SEEDS if ks not in seeds]
    for kind, seed in seeds:
        ref, hip, scalars, text = T.build(kind, seed, tmp)
        program = type(hip)._gt_program_
        kernels = {k.name: k for k in program.kernels}
        for geometry, domain, arrays, origins, case in T.cases(kind, seed, ref, hip, text):
            total[geometry] += 1
            if isinstance(case, G.LeftOut):
                left[geometry] += 1
                assert (geometry in G.ALIAS and "no two I-J-K fields" in str(case)) or (geometry == "sub_box" and "region" in str(case))
                continue
            vkey, lead, labels = T.census_case(program, ref.field_info, case)
            rows.append((kind, seed, geometry, case, vkey, lead, [(kernels[n], label) for n, label in labels]))
    return rows, left, total


def test_census_every_twin_under_both_kinds_of_lead_and_all_four_variants(census):
    rows, _, _ = census
    seen = collections.Counter()
    for kind, seed, geometry, case, vkey, lead, labels in rows:
        assert vkey == G.VARIANT[geometry], (kind, seed, geometry)
        for kern, label in labels:
            seen[("tc" if label.startswith("tc") else label, lead > 0)] += 1
    print(", ".join(f"{label} with{'' if led else 'out'} a lead: {n}" for (label, led), n in sorted(seen.items())))
    for label in (*LANE_TWINS, "tc"):
        assert seen[(label, False)] and seen[(label, True)], (label, dict(seen))
    assert seen[("point", False)]
    assert {vkey for _, _, _, _, vkey, _, _ in rows} == {(True, True), (True, False), (False, True), (False, False)}


def test_census_no_lane_twin_where_the_geometry_forbids_it(census):
    rows, _, _ = census
    for kind, seed, geometry, case, vkey, lead, labels in rows:
        bad = T.misplaced_lane_twins(case, {k.name: k for k, _ in labels}, [(k.name, label) for k, label in labels])
        assert not bad, (kind, seed, geometry, bad)
    # ... and the control does select them, so the above is no accident of the corpus
    assert sum(label in LANE_TWINS for _, _, g, _, _, _, labels in rows if g == "preset" for _, label in labels) >= 10


def test_cap_on_the_cases_left_out(census):
    _, left, total = census
    print({g: f"{left[g]} of {total[g]}" for g in G.GEOMETRIES})
    for geometry in G.GEOMETRIES:
        if geometry in (*G.ALIAS, "sub_box"):
            assert 5 * left[geometry] <= total[geometry], (geometry, left[geometry], total[geometry])
        else:
            assert left[geometry] == 0, geometry
