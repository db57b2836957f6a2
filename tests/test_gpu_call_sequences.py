"""Sequences of calls of one stencil object (tests/call_sequences.py) on the device: every call, whether the launch-plan cache serves
it or not, must leave every byte of every buffer the test owns as the `numpy` backend leaves the test's host mirror of it.

Per step the arrays of the call, and every other buffer the sequence has made (the buffers an array object pointed at before it was
re-pointed or replaced among them), are downloaded whole and compared bit for bit: halo, padding between the rows, the sign of a
zero; NaN as NaN.  Calls of `_prepare` (generic executor) and of `_lib.Field.make` (kernel library) are counted: what the model
calls a hit must be served without preparation, what it calls a miss for scalar bits, address or strides must not be.

A plan that is stale can only reach memory this file owns: every buffer lives as long as its sequence, the buffers an array
object moves between have one shape, and no allocator cache is emptied here.

Measured on one MI355X in one session: the whole file (17 objects, three sequences of 60 calls each, and the four-stream rounds) takes 12 s.

The helpers up to ``Runner`` need no device: tests/test_call_sequences.py runs its census over the same objects with them."""

import numpy as np
import pytest

import call_sequences as CS
import device_layouts
import fuzz_stencils
import stencil_zoo as zoo

DOMAINS = ((40, 9, 5), (33, 7, 3), (70, 5, 4))
SEEDS = (0, 1, 2)
LENGTH = 60
#: random programs of tests/fuzz_stencils.py whose generated kernels take scalars: structural 0 (`s0`, no scratch), 1 and 2 (`s0`,
#: scratch), 3 (`s0`, `s1`); typed 3 (`n`), 4, 9 and 14 (`n` and `s`)
STRUCTURAL_SEEDS = (0, 1, 2, 3)
TYPED_SEEDS = (3, 4, 9, 14)
OBJECTS = (["local_f64", "local_f32", "two_stage_written_input", "two_sweep_0"] + [f"structural_{s}" for s in STRUCTURAL_SEEDS]
           + [f"typed_{s}" for s in TYPED_SEEDS] + ["lap5_f32", "lap5_f64", "hdiff_field", "hdiff_scalar", "tridiag"])


def local_stencil(a: "Field[T]", b: "Field[T]", c: "Field[T]", out: "Field[T]", *, s: np.float64, n: np.int64):  # noqa: F821
    """A temporary read at a horizontal offset (`t`, in scratch: it depends on the written `b`), one assigned under a condition
    only (`m`), a float64 scalar as divisor and as factor, an integer scalar."""
    with computation(PARALLEL), interval(...):  # noqa: F821
        b = a * s  # noqa: F841
        t = b + a / s
        if a > 0.0:
            m = t[-1, 0, 0] * n
        if a > 0.0:
            out = t[1, 0, 0] + t[0, -1, 0] + m + c[0, 1, 0]  # noqa: F841
        else:
            out = t[1, 0, 0] - c[0, 1, 0] * s  # noqa: F841


_BUILT = {}


def build(name, tmp_path):
    """(numpy object, hip:mi300 object, Spec, oracle context, values kind) of an object under test; built once per process."""
    if name in _BUILT:
        return _BUILT[name]
    import contextlib

    import oracle.numpy_backend  # noqa: F401 - registers backend "numpy"
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_backend, hip_generic, hip_templates
    from test_oracle_independent import defined_casts_only

    context, typed, own, palette, domains = contextlib.nullcontext, False, {}, CS.FLOAT_PALETTE, DOMAINS
    alias, refusals, kw = None, (), {}
    if name.startswith("local_"):
        defn, kw = local_stencil, {"dtypes": {"T": np.dtype(name[6:].replace("f", "float"))}}
        alias, refusals = ("out", "a"), (("out", "c"), ("out", "b"))
    elif name == "two_stage_written_input":
        defn = zoo.two_stage_written_input
        refusals = (("out", "b"),)
    elif name.startswith(("two_sweep_", "structural_", "typed_")):
        kind, seed = name.rsplit("_", 1)
        make = {"structural": fuzz_stencils.make_stencil, "typed": fuzz_stencils.make_typed_stencil,
                "two_sweep": fuzz_stencils.make_two_sweep_stencil}[kind]
        defn, own, _ = make(int(seed), tmp_path)
        context, typed, palette = defined_casts_only, kind == "typed", CS.FINITE_PALETTE
    elif name.startswith("lap5_"):
        defn, kw = hip_templates.lap_notebook, {"dtypes": {"T": np.dtype(name[5:].replace("f", "float"))}}
        refusals = (("out", "inp"),)
    elif name == "hdiff_field":
        defn, kw = hip_templates.hdiff_limiter_field, {"dtypes": {"T": np.float64}}
        alias, refusals = ("out_field", "coeff"), (("out_field", "in_field"),)
    elif name == "hdiff_scalar":
        defn, kw = hip_templates.hdiff_limiter_scalar, {"dtypes": {"T": np.float64, "S": np.float64}}
        refusals = (("out_field", "in_field"),)
    elif name == "tridiag":
        defn, kw = hip_templates.tridiagonal_solver, {"dtypes": {"T": np.float64}}
        alias, refusals = ("out", "rhs"), (("sup", "rhs"),)
    ref = gtscript.stencil(backend="numpy", definition=defn, **kw)
    hip = gtscript.stencil(backend="hip:mi300", definition=defn, **kw)
    generic = isinstance(hip, hip_generic.HipGenericStencilObject)
    fields = tuple(n for n, i in hip.field_info.items() if i is not None)
    keyed = fields
    if generic:
        program = type(hip)._gt_program_
        keyed = tuple(d.name for d in program.plan.api_fields)  # (a field the program never touches is no part of a plan)
        params = {p.name: str(np.dtype(p.dtype)) for p in program.plan.params}
        scratch = bool(program.plan.scratch)
        if name.startswith("two_sweep_"):  # its shallowest `_tc<n>` twin and the plain kernel, one level below
            k = max(kern.top_cache[-1][2] for kern in program.kernels if kern.top_cache)
            domains = ((40, 9, k), (33, 7, k - 1), (70, 5, k))
    else:
        assert isinstance(hip, hip_backend.HipStencilObject), name
        params, scratch = {n: str(np.dtype(i.dtype)) for n, i in hip.parameter_info.items() if i is not None}, False
    spec = CS.Spec(name, fields, domains, {p: d for p, d in params.items() if d.startswith("float")},
                   {p: d for p, d in params.items() if not d.startswith("float")}, generic, scratch, alias, refusals,
                   tuple(palette), {p: v for p, v in own.items() if p in params}, keyed)
    fixed = {p: v for p, v in own.items() if p not in params}  # parameters of the signature that the program does not use
    _BUILT[name] = (ref, hip, spec, context, typed, fixed)
    return _BUILT[name]


def sequences(spec):
    return [CS.make_sequence(spec, seed, LENGTH) for seed in SEEDS]


def geometry_of(hip, domains):
    """Per field (shape, the two origins): room for the largest domain, the stencil's boundary (the widest of all fields, so that
    fields of one dtype are alike and can stand in for each other) and the second origin, which lies one column further in; the
    first has its column on a multiple of 4 items, i.e. on a 16-byte boundary of a buffer that starts on one."""
    infos = {n: i for n, i in hip.field_info.items() if i is not None}
    lo = [max(max(0, int(i.boundary[ax][0])) for i in infos.values()) for ax in range(3)]
    hi = [max(max(0, int(i.boundary[ax][1])) for i in infos.values()) for ax in range(3)]
    lo[0] = -(-lo[0] // 4) * 4
    big = [max(d[ax] for d in domains) for ax in range(3)]
    out = {}
    for n, i in infos.items():
        axes = ["IJK".index(a) for a in i.axes]
        shape = tuple(big[ax] + lo[ax] + hi[ax] + (1 if ax == 0 else 0) for ax in axes) + tuple(int(d) for d in i.data_dims)
        first = tuple(lo[ax] for ax in axes) + (0,) * len(i.data_dims)
        second = tuple(lo[ax] + (1 if ax == 0 else 0) for ax in axes) + (0,) * len(i.data_dims)
        out[n] = (shape, (first, second if "I" in i.axes else first))
    return out


def item_strides(shape, padded: bool):
    """Strides in items, the first axis fastest, its rows padded to 32 items (``padded``: and 32 more); -> (strides, items)."""
    pitch = -(-shape[0] // 32) * 32 + (32 if padded else 0)
    strides, acc = [], 1
    for n, extent in enumerate(shape):
        strides.append(acc)
        acc *= pitch if n == 0 else extent
    return tuple(strides), acc


def twins_reached(hip, domains):
    """Without a device: the labels `select_twin` gives over the domains, both origins, with and without an alias, and the largest
    number of workgroups of a launch."""
    from gt4py_amd.cartesian.backend import hip_generic
    from test_gpu_fuzz_geometries import FAKE_BASE, scratch_geometry

    program = type(hip)._gt_program_
    geo = geometry_of(hip, domains)
    labels, groups = set(), 0
    for domain in domains:
        for which in (0, 1):
            for no_alias in (True, False):
                geometry = {}
                for n, (shape, origins) in geo.items():
                    info = hip.field_info[n]
                    isz = np.dtype(info.dtype).itemsize
                    st = dict(zip(info.axes, item_strides(shape, False)[0]))
                    ptr = FAKE_BASE + (len(geometry) + 1) * (1 << 26) + sum(o * s for o, s in zip(origins[which], st.values())) * isz
                    geometry[n] = (ptr, st.get("J", 0), st.get("K", 0), isz)
                geometry.update(scratch_geometry(program, domain, FAKE_BASE))
                for kern in program.kernels:
                    twins = (bool(kern.vec), bool(getattr(kern, "shared_halo", 0)) and no_alias,
                             tuple((n_reg, min_k) for n_reg, _, min_k in (kern.top_cache or ())) if no_alias else ())
                    label, grid, _ = hip_generic.select_twin(kern, twins, which, no_alias, geometry, domain,
                                                             1 if kern.plane is not None else None)
                    if label is not None:
                        labels.add(label)
                        groups = max(groups, grid[0] * grid[1] * grid[2])
    return labels, groups


# ---- the device ------------------------------------------------------------------------------------------------------------------
class Buffer:
    """A flat device buffer with a strided view in it, and the host image of all of it."""

    def __init__(self, shape, dtype, padded, values):
        import torch

        from gt4py_amd.storage.device_array import torch_dtype

        self.dtype = np.dtype(dtype)
        self.shape = tuple(shape)
        self.strides, items = item_strides(shape, padded)
        isz = self.dtype.itemsize
        fill = device_layouts.SENTINEL[isz] if isz in (4, 8) else {1: 0xA5, 2: 0x7DAD}[isz]
        self.image = np.full(items + 8, fill, dtype=device_layouts.NP_UINT[isz]).view(np.uint8).view(self.dtype)
        self.host()[...] = values
        self.flat = torch.empty(items + 8, dtype=torch_dtype(self.dtype), device="cuda")
        self.upload()

    def view(self):
        """A tensor of its own on the buffer: re-pointing the tensor of an array object must not move anyone else's."""
        import torch

        return torch.as_strided(self.flat, self.shape, self.strides)

    def host(self):
        return np.lib.stride_tricks.as_strided(self.image, self.shape, tuple(s * self.dtype.itemsize for s in self.strides))

    def upload(self):
        import torch

        self.flat.copy_(torch.from_numpy(self.image.view(np.uint8)).cuda().view(self.flat.dtype))

    def check(self, what):
        got = self.flat.cpu().view(__import__("torch").uint8).numpy().view(device_layouts.NP_UINT[self.dtype.itemsize])
        want = self.image.view(device_layouts.NP_UINT[self.dtype.itemsize])
        ok = got == want
        if self.dtype.kind == "f":
            ok |= np.isnan(got.view(self.dtype)) & np.isnan(self.image)
        if not ok.all():
            bad = np.flatnonzero(~ok)
            raise AssertionError(f"{what}: {bad.size} items of the whole buffer differ, first at flat index {bad[:6].tolist()} "
                                 f"(shape {self.shape}, strides {self.strides}); got {got.view(self.dtype)[bad[:6]].tolist()}, "
                                 f"want {self.image[bad[:6]].tolist()}")


class Runner:
    """One sequence on the device."""

    def __init__(self, name, tmp_path, streams, monkeypatch, seed):
        from gt4py_amd import _lib
        from gt4py_amd.cartesian.backend import hip_generic

        self.ref, self.hip, self.spec, self.context, self.typed, self.fixed = build(name, tmp_path)
        self.streams = streams
        self.rng = np.random.default_rng([seed, len(name)])
        self.geo = geometry_of(self.hip, self.spec.domains)
        self.arrays = {}  # (field, slot) -> [DeviceArray, [Buffer] * BUFFERS, current buffer]
        self.every = []  # every buffer this sequence made, for as long as it runs
        for f in self.spec.fields:
            for s in range(CS.SLOTS):
                self.new_array(f, s)
        self.frozen = {}
        self.prepared = 0
        cls = type(self.hip)
        cls._gt_launch_cache_.clear()
        if self.spec.generic:
            cls._gt_scratch_.clear()
            inner = hip_generic.HipGenericStencilObject._prepare

            def counting(obj, *args, **kwargs):
                self.prepared += 1
                return inner(obj, *args, **kwargs)

            monkeypatch.setattr(hip_generic.HipGenericStencilObject, "_prepare", counting)
        else:
            inner = _lib.Field.make.__func__

            def counting(klass, *args, **kwargs):
                self.prepared += 1
                return inner(klass, *args, **kwargs)

            monkeypatch.setattr(_lib.Field, "make", classmethod(counting))

    def values(self, field, shape):
        dt, rng = np.dtype(self.hip.field_info[field].dtype), self.rng
        if dt.kind == "f":
            if self.typed:
                return np.where(rng.random(shape) < 0.25, rng.integers(-6, 7, shape) * 0.5, rng.uniform(-3.0, 3.0, shape)).astype(dt)
            return (rng.uniform(-1.0, 1.0, shape) + (4.5 if field == "diag" else 0.0)).astype(dt)
        if dt.kind == "i":
            return (rng.integers(-1, 2, shape) if field == "idx" else rng.integers(-50, 51, shape)).astype(dt)
        return rng.integers(0, 2, shape).astype(dt)

    def new_array(self, field, slot):
        from gt4py_amd.storage.device_array import DeviceArray

        shape = self.geo[field][0]
        dt = self.hip.field_info[field].dtype
        bufs = [Buffer(shape, dt, b == CS.BUFFERS - 1, self.values(field, shape)) for b in range(CS.BUFFERS)]
        self.every += bufs
        self.arrays[field, slot] = [DeviceArray(bufs[0].view()), bufs, 0]

    def mutate(self, kind, field, slot, buffer):
        import torch

        entry = self.arrays[field, slot]
        if kind == "refill":
            buf = entry[1][entry[2]]
            buf.host()[...] = self.values(field, buf.shape)
            buf.upload()
        elif kind == "replace":
            old_id = id(entry[0])
            del entry[0]  # the only reference to the object; its buffers stay in self.every
            del self.arrays[field, slot]
            for _ in range(4):  # (bounded) the next object of this size often gets the address of the last one freed
                self.new_array(field, slot)
                if id(self.arrays[field, slot][0]) == old_id:
                    break
        else:  # repoint, repitch: the same object on another buffer, the usual torch way
            new = entry[1][buffer]
            if kind == "repoint":
                entry[0].tensor.data = new.view()
            else:
                entry[0].tensor.set_(new.flat.untyped_storage(), 0, new.shape, new.strides)
            entry[2] = buffer
            assert entry[0].ptr == new.flat.data_ptr() and entry[0].strides == tuple(s * new.dtype.itemsize for s in new.strides)
        torch.cuda.synchronize()

    def step(self, step, what):
        import contextlib

        import torch

        spec = self.spec
        if step.mutation:
            self.mutate(*step.mutation)
        given = {f: (step.same_as[1] if step.same_as and step.same_as[0] == f else f) for f in spec.fields}
        entries = {f: self.arrays[given[f], step.slots[given[f]]] for f in spec.fields}
        origin = {f: self.geo[f][1][step.origin[f]] for f in spec.fields}
        scalars = {**self.fixed, **step.scalars}
        exact = all(np.dtype(type(v)) == np.dtype(self.hip.parameter_info[p].dtype) for p, v in scalars.items())
        info = {} if step.path.endswith("+info") else None
        before = self.prepared
        with contextlib.ExitStack() as stack:
            if step.stream:
                stack.enter_context(torch.cuda.stream(self.streams[step.stream - 1]))
            if step.refused:
                stack.enter_context(pytest.raises((ValueError, RuntimeError), match="overlap in memory|same array"))
            if step.path.startswith("frozen"):
                key = (step.domain, tuple(sorted(origin.items())))
                if key not in self.frozen:
                    self.frozen[key] = self.hip.freeze(origin=origin, domain=step.domain)
                self.frozen[key](**{f: e[0] for f, e in entries.items()}, **scalars, **({"exec_info": info} if info is not None else {}))
            else:
                self.hip(**{f: e[0] for f, e in entries.items()}, **scalars, origin=origin, domain=step.domain, validate_args=exact,
                         exec_info=info)
        torch.cuda.synchronize()
        if not step.refused:
            typed = {p: np.dtype(self.hip.parameter_info[p].dtype).type(v) for p, v in scalars.items()}
            with self.context():
                self.ref(**{f: e[1][e[2]].host() for f, e in entries.items()}, **typed, origin=origin, domain=step.domain)
            if info is not None:
                assert info["run_end_time"] >= info["run_start_time"], what
        for n, buf in enumerate(self.every):  # the call's arrays, its inputs, and every buffer an object pointed at before
            buf.check(f"{what}: buffer {n} of the sequence")
        cls = type(self.hip)
        assert len(cls._gt_launch_cache_) <= 8, what
        if spec.generic:
            from gt4py_amd.cartesian.backend import hip_generic

            kept = list(cls._gt_scratch_)
            assert len({k[0] for k in kept}) <= hip_generic.MAX_SCRATCH_STREAMS, f"{what}: scratch kept for {kept}"
            assert len({k[0] for k in kept}) == len(kept), f"{what}: more than one domain per stream in {kept}"
        return self.prepared > before


@pytest.fixture(scope="module")
def streams():
    import torch

    return [torch.cuda.Stream() for _ in range(CS.STREAMS - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", OBJECTS)
def test_every_call_of_a_sequence_leaves_what_a_fresh_call_would(name, tmp_path, streams, monkeypatch):
    _, hip, spec, *_ = build(name, tmp_path)
    if name.startswith("local_") or name == "two_stage_written_input":
        assert type(hip)._gt_program_.plan.scratch, "the object must keep a temporary in scratch memory"
    for seed, steps in zip(SEEDS, sequences(spec)):
        run = Runner(name, tmp_path, streams, monkeypatch, seed)
        served, hits, may_miss = 0, 0, 0
        for n, step in enumerate(steps):
            what = f"{name}, seed {seed}, step {n} ({step.kind}, {step.path}, stream {step.stream}, domain {step.domain}, " \
                   f"scalars {step.scalars}, model: {'hit' if step.hit else 'miss for ' + str(step.cause)})"
            prepared = run.step(step, what)
            if step.refused:
                continue
            served += not prepared
            hits += step.hit
            may_miss += step.may_miss
            assert prepared or step.cause not in ("scalar bits", "address", "strides"), f"{what}: served without preparation"
        assert served >= hits - may_miss, f"{name}, seed {seed}: {served} calls served without preparation, the model has {hits} hits"
        monkeypatch.undo()
        type(hip)._gt_launch_cache_.clear()


@pytest.mark.gpu
def test_four_streams_enqueued_back_to_back(tmp_path, streams):
    """Three rounds of four calls on four streams and disjoint arrays, enqueued without a synchronisation between them."""
    import torch

    import oracle.numpy_backend  # noqa: F401
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.storage.device_array import DeviceArray

    kw = {"dtypes": {"T": np.float64}}
    ref = gtscript.stencil(backend="numpy", definition=local_stencil, **kw)
    hip = gtscript.stencil(backend="hip:mi300", definition=local_stencil, device_sync=False, **kw)
    geo = geometry_of(hip, DOMAINS)
    rng = np.random.default_rng(5)
    sets = [{f: Buffer(shape, np.float64, False, rng.uniform(-1, 1, shape)) for f, (shape, _) in geo.items()} for _ in range(4)]
    devs = [{f: DeviceArray(b.view()) for f, b in one.items()} for one in sets]
    for round_ in range(3):
        calls = []
        for n, one in enumerate(sets):
            one["a"].host()[...] = rng.uniform(-1, 1, one["a"].shape)
            one["a"].upload()
            calls.append((DOMAINS[(n + round_) % 3], {f: o[(n + round_) % 2] for f, (_, o) in geo.items()}, {"s": [1.5, -0.0, 0.0, -2.0][n], "n": n - 1}))
        torch.cuda.synchronize()
        for n, (domain, origin, scalars) in enumerate(calls):
            with torch.cuda.stream(streams[n]):
                hip(**devs[n], s=scalars["s"], n=np.int64(scalars["n"]), origin=origin, domain=domain)
        torch.cuda.synchronize()
        for n, (domain, origin, scalars) in enumerate(calls):
            ref(**{f: b.host() for f, b in sets[n].items()}, s=np.float64(scalars["s"]), n=np.int64(scalars["n"]), origin=origin, domain=domain)
            for f, b in sets[n].items():
                b.check(f"round {round_}, stream {n}, field {f}")
