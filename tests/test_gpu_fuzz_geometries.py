"""Random programs of the generic executor across the storage geometries of tests/stencil_geometries.py, byte for byte.

Per seed the program is built for `numpy` and for `hip:mi300`; on both domains and in every geometry the `hip:mi300` object runs on
strided views of flat device buffers, and every byte of every buffer is compared with the sentinel image that holds the numpy
oracle's arrays in the views.  The launches the call prepared must carry the function handles of the twins that
`hip_generic.select_twin` names for the geometry the TEST computed (pointers, strides, lead and aliasing worked out here, not read
from the product), and the compiled variant must be the one the geometry is there to select.

Measured on one MI355X in one session: the median seed of test_fuzz_codegen.py's
test_generated_kernels_match_the_oracle_on_random_stencils takes 0.15 s, that file's GPU tests 161 s; a seed here (up to four
compiled variants, 24 calls, every buffer downloaded) takes 0.56 s in the median and 1.2 s at most, a two-sweep seed on its 58
levels 3 s, the whole file 46 s -- within four times that median plus half for the downloads, so the seed counts stay at 40 structural and 24 typed, plus the named seeds.

The helpers up to ``run_case`` need no device: tests/test_stencil_geometries.py runs its census over the same seeds with them."""

import os

import numpy as np
import pytest

import fuzz_stencils
import stencil_geometries as G
import stencil_zoo as zoo

_N = int(os.environ.get("GT4MI_FUZZ_SEEDS", "0"))
_FIRST = int(os.environ.get("GT4MI_FUZZ_FIRST_SEED", "0"))
STRUCTURAL_SEEDS = list(range(_FIRST, _FIRST + (_N or 40)))
TYPED_SEEDS = list(range(_FIRST, _FIRST + (_N or 24)))
#: seeds beyond the default range that the census (test_stencil_geometries.py) needs to see every label under both kinds of lead,
#: and seeds kept as regression cases of findings: (kind, seed)
NAMED_SEEDS = [("two_sweep", 0), ("two_sweep", 1)]  # Thomas-like column programs on a deep domain: the only ones with `_tc<n>` twins
FAKE_BASE = 0x7F00_0000_0000  # addresses of the census' buffers: far above 2^32, on a 4 MiB boundary like fresh device blocks


def build(kind, seed, tmp_path):
    """(numpy object, hip:mi300 object, scalars, program text) of a structural, typed or two-sweep seed."""
    import oracle.numpy_backend  # noqa: F401 - registers backend "numpy"
    from gt4py_amd.cartesian import gtscript

    make = {"structural": fuzz_stencils.make_stencil, "typed": fuzz_stencils.make_typed_stencil,
            "two_sweep": fuzz_stencils.make_two_sweep_stencil}[kind]
    defn, scalars, text = make(seed, tmp_path)
    return gtscript.stencil(backend="numpy", definition=defn), gtscript.stencil(backend="hip:mi300", definition=defn), scalars, text


def fit(kind, domain, ref, text, hip=None):
    """test_fuzz_codegen._fit: K at least the program's minimum, I and J at least 6 where a horizontal region needs it; typed
    programs get a third level (their run-time K indices are clipped to 0..2), two-sweep programs as many as their shallowest
    top-of-column cache asks for."""
    ni, nj, nk = domain
    if "region[" in text:
        ni, nj = max(ni, 6), max(nj, 6)
    if kind == "two_sweep":
        nk = max([nk] + [k.top_cache[-1][2] for k in type(hip)._gt_program_.kernels if k.top_cache])
    return (ni, nj, max(nk, ref.domain_info.min_sequential_axis_size, 3 if kind == "typed" else 0))


def written_fields(hip):
    from gt4py_amd.cartesian.backend import hip_generic

    return hip_generic._access_profile(type(hip)._gt_program_.plan)[0]


def cases(kind, seed, ref, hip, text):
    """(domain, arrays, origins, Case or LeftOut) for both domains and every geometry."""
    make = zoo.make_typed_inputs if kind == "typed" else zoo.make_inputs
    for domain in G.DOMAINS:
        domain = fit(kind, domain, ref, text, hip)
        arrays, origins = make(ref, domain, seed)
        for geometry in G.GEOMETRIES:
            try:
                case = G.Case(geometry, arrays, origins, ref.field_info, written_fields(hip), domain,
                              region_reach=6 if "region[" in text else 0, used={d.name for d in type(hip)._gt_program_.plan.api_fields})
            except G.LeftOut as reason:
                case = reason
            yield geometry, domain, arrays, origins, case


class Oracle:
    """The numpy object's whole arrays, computed once per (domain, origins)."""

    def __init__(self, kind, ref, scalars):
        self.kind, self.ref, self.scalars, self.known = kind, ref, scalars, {}

    def __call__(self, case, arrays):
        from test_oracle_independent import defined_casts_only

        key = (case.domain, tuple(sorted(case.origins.items())))
        if key not in self.known:
            expect = {k: v.copy() for k, v in arrays.items()}
            with defined_casts_only():
                self.ref(**expect, **self.scalars, origin=case.origins, domain=case.domain)
            self.known[key] = expect
        return self.known[key]


def common_lead(geometry, names):
    """The rule of HipGenericStencilObject._prepare, restated: items by which the origins of the fields with an I axis lie past a
    16-byte boundary when that is one number for all of them (fields of 1 or 2 bytes never agree with the others), else 0."""
    leads = set()
    for n in names:
        ptr, _, _, isz = geometry[n]
        leads.add((ptr % 16) // isz if isz in (4, 8) else None)
    lead = leads.pop() if len(leads) == 1 else 0
    return lead or 0


def launch_labels(program, twins_of, lead, no_alias, geometry, domain):
    """[(kernel, label)] of every launch of a call, in launch order: `select_twin` per kernel, the kernels of a block the host runs
    plane by plane once per level."""
    from gt4py_amd.cartesian.backend import hip_generic

    out, kernels, n = [], program.kernels, 0
    while n < len(kernels):
        kern = kernels[n]
        if kern.plane is None:
            label = hip_generic.select_twin(kern, twins_of(n), lead, no_alias, geometry, domain)[0]
            out += [(kern.name, label)] if label is not None else []
            n += 1
            continue
        m = n
        while m < len(kernels) and kernels[m].plane is not None and kernels[m].plane[0] == kern.plane[0]:
            m += 1
        k0, k1 = kern.plane[2].range(domain[2])
        body = [(kernels[x].name, hip_generic.select_twin(kernels[x], twins_of(x), lead, no_alias, geometry, domain, 1)[0]) for x in range(n, m)]
        out += [b for _ in range(k0, k1) for b in body if b[1] is not None]
        n = m
    return out


def misplaced_lane_twins(case, kernels, labels):
    """The launches of `labels` that a geometry must keep from the 16-byte-lane twins, by the geometry's own statement and by no
    code of the product: none at all where the I stride is not 1 or the arguments alias; none for a stage whose lane fields
    include a field of an odd pitch or plane, or the one field that `mixed_lead` moved off its column."""
    affected = {"mixed_lead": {case.off_column}, "odd_pitch": set(case.fields), "odd_plane": set(case.fields)}.get(case.geometry)
    bad = []
    for name, label in labels:
        if label not in ("vec", "vecs"):
            continue
        fields = set(kernels[name].vec_fields if label == "vec" else kernels[name].shared_fields)
        if not all(G.VARIANT[case.geometry]) or (affected is not None and affected & fields):
            bad.append((name, label))
    return bad


def scratch_geometry(program, domain, base):
    """The geometry tuples of the temporaries kept in memory, for a scratch buffer at ``base`` (a 4 MiB boundary)."""
    from gt4py_amd.cartesian.backend import hip_generic

    axes = {t.name: t.axes for t in program.plan.stencil.temporaries}
    return {name: (base + off + (oi + oj * ni) * isz, ni, ni * nj if "K" in axes[name] else 0, isz)
            for name, (off, ni, nj, isz, oi, oj) in hip_generic.scratch_layout(program.plan, domain)[0].items()}


def census_case(program, field_info, case):
    """Without a device: (variant key, lead, [(kernel, label)]) of a case, buffers at made-up addresses, `_tc` twins taken as
    present where the kernel record offers them, `from_array` storage as storage/allocators.plan_buffer lays it out."""
    from gt4py_amd.storage import allocators, layout

    names = list(case.buffers) + list(case.plain)
    ptr_of = {b: FAKE_BASE + (n + 1) * (1 << 26) for n, b in enumerate(names)}
    case.resolve(ptr_of)
    geometry = {k: (case.origin_pointer(ptr_of, k), s[1], s[2], case.dtype[k].itemsize) for k, (_, _, s) in case.fields.items()}
    preset = layout.from_name("hip:mi300")
    unit_i = all(s[0] == 1 for _, _, s in case.fields.values())
    for k, aligned in case.plain.items():
        info = field_info[k]
        dims = tuple(info.axes) + tuple(str(n) for n in range(len(info.data_dims)))
        plan = allocators.plan_buffer(case.shape[k], case.dtype[k], preset["layout_map"](dims), preset["alignment_bytes"], aligned)
        byte = dict(zip(dims, plan.strides))
        isz = case.dtype[k].itemsize
        ptr = ptr_of[k] + plan.byte_offset(ptr_of[k]) + sum(o * s for o, s in zip(case.origins[k], plan.strides))
        geometry[k] = (ptr, byte.get("J", 0) // isz, byte.get("K", 0) // isz, isz)
    geometry.update(scratch_geometry(program, case.domain, FAKE_BASE))
    spans = sorted(case.span(ptr_of, k) for k in case.fields)
    no_alias = all(spans[n][1] <= spans[n + 1][0] for n in range(len(spans) - 1))
    lead = common_lead(geometry, [d.name for d in program.plan.api_fields if "I" in d.axes])

    def twins_of(n):
        kern = program.kernels[n]
        return (bool(kern.vec) and unit_i, bool(kern.shared_halo) and unit_i and no_alias,
                tuple((n_reg, min_k) for n_reg, _, min_k in (kern.top_cache or ())) if no_alias else ())

    return (unit_i, no_alias), lead, launch_labels(program, twins_of, lead, no_alias, geometry, case.domain)


# ---- the device ------------------------------------------------------------------------------------------------------------------
def run_case(kind, seed, hip, scalars, text, geometry_name, arrays, case, oracle):
    import warnings

    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian.backend import hip_generic
    from test_oracle_independent import assert_same_bits

    what = f"{kind} seed {seed}, geometry {geometry_name}, domain {case.domain}, origins {case.origins}"
    cls = type(hip)
    program = cls._gt_program_
    info = hip.field_info
    dev = G.DeviceCase(case, arrays)
    plain = {k: gt_storage.from_array(arrays[k], dtype=arrays[k].dtype, backend="hip:mi300", aligned_index=aligned,
                                      dimensions=tuple(info[k].axes) + tuple(str(n) for n in range(len(info[k].data_dims))))
             for k, aligned in case.plain.items()}
    expect = oracle(case, arrays)
    cls._gt_launch_cache_.clear()  # the entry this call prepares is then the only one
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the layout warning of the reference, where the geometry is not the preset's
            hip(**dev.views, **plain, **scalars, origin=case.origins, domain=case.domain)
    except ValueError as refusal:
        raise AssertionError(f"{what}: refused: {refusal}\n{text}") from refusal
    torch.cuda.synchronize()
    # 1. every byte
    try:
        case.compare(dev.before, expect, dev.download(), what)
    except AssertionError as diff:
        raise AssertionError(f"{diff}\n{text}") from None
    for k, d in plain.items():
        assert_same_bits(d.get(), expect[k], f"{what}: field {k}\n{text}")
    # 2. the twins that ran, against the geometry as this test knows it
    (_, args, launches, keep), = cls._gt_launch_cache_.values()
    vkey, ran = keep[3]
    assert vkey == G.VARIANT[geometry_name], f"{what}: variant {vkey}, the geometry is there to select {G.VARIANT[geometry_name]}\n{text}"
    variant = cls._gt_variants_[vkey]
    geometry = {k: (case.origin_pointer(dev.ptr_of, k), s[1], s[2], case.dtype[k].itemsize) for k, (_, _, s) in case.fields.items()}
    for k, d in plain.items():
        byte = dict(zip(info[k].axes, d.strides))
        ptr = d.ptr + sum(o * s for o, s in zip(case.origins[k], d.strides))
        geometry[k] = (ptr, byte.get("J", 0) // d.itemsize, byte.get("K", 0) // d.itemsize, d.itemsize)
    if program.plan.scratch:
        (buf, _), = [v for key, v in cls._gt_scratch_.items() if key[1:] == case.domain]
        period = hip_generic.PLACEMENT_PERIOD
        geometry.update(scratch_geometry(program, case.domain, -(-buf.data_ptr() // period) * period))
    lead = common_lead(geometry, [d.name for d in program.plan.api_fields if "I" in d.axes])
    assert args.lead == lead, f"{what}: the call's lead is {args.lead}, the origins' common lead {lead}\n{text}"

    def twins_of(n):
        return (variant.vec_functions[n] is not None, variant.shared_functions[n] is not None,
                tuple((n_reg, min_k) for n_reg, (_, min_k) in zip(variant.tc_levels[n], variant.tc_functions[n])))

    want = launch_labels(program, twins_of, lead, vkey[1], geometry, case.domain)
    assert ran == want, f"{what}: launched {ran}, the geometry selects {want}\n{text}"
    bad = misplaced_lane_twins(case, {k.name: k for k in program.kernels}, ran)
    assert not bad, f"{what}: lane twins launched that the geometry must keep out: {bad}\n{text}"
    index = {kern.name: n for n, kern in enumerate(program.kernels)}
    for (fn, _, _, _), (name, label) in zip(launches, ran):
        n = index[name]
        handle = {"point": variant.functions[n], "vec": variant.vec_functions[n], "vecs": variant.shared_functions[n]}.get(label)
        if handle is None:
            handle = variant.tc_functions[n][variant.tc_levels[n].index(int(label[2:]))][0]
        assert fn.value == handle.value, f"{what}: the launch of {name} does not carry the `{label}` function\n{text}"
    return vkey, lead, ran


def _run_seed(kind, seed, tmp_path):
    ref, hip, scalars, text = build(kind, seed, tmp_path)
    oracle = {}
    for geometry, domain, arrays, origins, case in cases(kind, seed, ref, hip, text):
        if isinstance(case, G.LeftOut):
            continue  # (counted and capped by test_stencil_geometries.py)
        run_case(kind, seed, hip, scalars, text, geometry, arrays, case, oracle.setdefault(domain, Oracle(kind, ref, scalars)))
    assert set(type(hip)._gt_variants_) <= {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", STRUCTURAL_SEEDS + [s for k, s in NAMED_SEEDS if k == "structural" and s not in STRUCTURAL_SEEDS])
def test_structural_programs_in_every_geometry_byte_for_byte(seed, tmp_path):
    _run_seed("structural", seed, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", TYPED_SEEDS + [s for k, s in NAMED_SEEDS if k == "typed" and s not in TYPED_SEEDS])
def test_typed_programs_in_every_geometry_byte_for_byte(seed, tmp_path):
    _run_seed("typed", seed, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [s for k, s in NAMED_SEEDS if k == "two_sweep"])
def test_two_sweep_programs_in_every_geometry_byte_for_byte(seed, tmp_path):
    _run_seed("two_sweep", seed, tmp_path)
