"""Differential fuzzing of the generic executor with random stencils (tests/fuzz_stencils.py).

CPU: the planner's rewritten IR (inlined temporaries, SSA versions) must evaluate, under the numpy oracle,
to the same bits as the original program, and the generated HIP must compile.  GPU: generated kernels vs
the oracle on every array.  Seeds are fixed, so a failure reproduces; the offending source is printed.
"""

import numpy as np
import pytest

import fuzz_stencils
import stencil_zoo as zoo

import os

# GT4MI_FUZZ_SEEDS=<n> widens both sweeps (one-off campaigns; results under profiles/)
_N = int(os.environ.get("GT4MI_FUZZ_SEEDS", "0"))
_FIRST = int(os.environ.get("GT4MI_FUZZ_FIRST_SEED", "0"))  # campaigns on fresh programs: seeds _FIRST .. _FIRST + _N - 1
CPU_SEEDS = list(range(_FIRST, _FIRST + (_N or 150)))
GPU_SEEDS = list(range(_FIRST, _FIRST + (_N or 200)))
DOMAINS = [(9, 7, 5), (66, 5, 4), (3, 3, 2)]


def _fit(domain, stencil_object, text):
    """Domains the program is valid on: K at least the stencil's minimum; with horizontal regions anchored
    at one edge (`: I[0] + 3`) the domain must be wider than the region's reach -- on a 3-wide domain such a
    region touches the far edge and its offset reads leave the array, in the reference just the same."""
    ni, nj, nk = domain
    if "region[" in text:
        ni, nj = max(ni, 6), max(nj, 6)
    return (ni, nj, max(nk, stencil_object.domain_info.min_sequential_axis_size))


def _build(seed, tmp_path, backend):
    import oracle.numpy_backend  # noqa: F401 - registers backend "numpy"
    from gt4py_amd.cartesian import gtscript

    defn, scalars, text = fuzz_stencils.make_stencil(seed, tmp_path)
    return gtscript.stencil(backend=backend, definition=defn), scalars, text


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_rewritten_ir_matches_original_under_the_oracle(seed, tmp_path):
    import oracle.numpy_backend as oracle_backend
    from gt4py_amd import _lib
    from gt4py_amd.cartesian import analysis

    ref, scalars, text = _build(seed, tmp_path, "numpy")
    hip, _, _ = _build(seed, tmp_path, "hip:mi300")
    program = getattr(type(hip), "_gt_program_", None)
    assert program is not None, text
    assert ref.field_info == hip.field_info
    domain = _fit(DOMAINS[seed % len(DOMAINS)], ref, text)
    arrays, origins = zoo.make_inputs(ref, domain, seed)
    expect = {k: v.copy() for k, v in arrays.items()}
    ref(**expect, **scalars, origin=origins, domain=domain)
    got = {k: v.copy() for k, v in arrays.items()}
    rewritten = program.plan.stencil
    oracle_backend.run_stencil(rewritten, analysis.compute_extents(rewritten), domain, origins, got, scalars)
    for k in arrays:
        np.testing.assert_array_equal(got[k], expect[k], err_msg=f"seed {seed}, field {k}\n{text}")
    if seed % 6 == 0:  # compile a sample (hiprtc takes ~0.3 s per program)
        assert _lib.rtc_compile(program.source, f"fuzz_{seed}.hip", ["-DGT4MI_UNIT_I_STRIDE=1", "-DGT4MI_NO_ALIAS=1"])[:4] == b"\x7fELF"


@pytest.mark.gpu
@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_generated_kernels_match_the_oracle_on_random_stencils(seed, tmp_path):
    import gt4py_amd.storage as gt_storage

    ref, scalars, text = _build(seed, tmp_path, "numpy")
    hip, _, _ = _build(seed, tmp_path, "hip:mi300")
    for domain in (DOMAINS[seed % len(DOMAINS)], (130, 9, 6)):
        domain = _fit(domain, ref, text)
        arrays, origins = zoo.make_inputs(ref, domain, seed)
        expect = {k: v.copy() for k, v in arrays.items()}
        ref(**expect, **scalars, origin=origins, domain=domain)
        dev = {k: gt_storage.from_array(v, dtype=v.dtype, backend="hip:mi300", aligned_index=origins[k],
                                        dimensions=tuple(hip.field_info[k].axes) + tuple(str(n) for n in range(len(hip.field_info[k].data_dims))))
               for k, v in arrays.items()}
        hip(**dev, **scalars, origin=origins, domain=domain)
        for k in arrays:
            np.testing.assert_array_equal(dev[k].get(), expect[k], err_msg=f"seed {seed} {domain}, field {k}\n{text}")


# ---- two-sweep column programs: the top-of-column cache of the code generator (stage_planner.TopCache) -----------
TWO_SWEEP_SEEDS = list(range(_FIRST, _FIRST + (_N or 60)))


def _two_sweep(seed, tmp_path, backend, **opts):
    import oracle.numpy_backend  # noqa: F401
    from gt4py_amd.cartesian import gtscript

    defn, scalars, text = fuzz_stencils.make_two_sweep_stencil(seed, tmp_path)
    return gtscript.stencil(backend=backend, definition=defn, **opts), scalars, text


@pytest.mark.parametrize("seed", TWO_SWEEP_SEEDS[::3])
def test_two_sweep_programs_plan_and_compile(seed, tmp_path):
    """CPU: most random Thomas-like programs qualify for the cache, and the `_tc` kernel compiles (shallow depths, so
    that every range is emitted)."""
    from gt4py_amd import _lib
    from gt4py_amd.cartesian.backend import hip_codegen

    saved = hip_codegen.TUNING["top_cache"]
    hip_codegen.TUNING["top_cache"] = (3, 4 * 8 * 3 * 256)
    try:
        hip, _, text = _two_sweep(seed, tmp_path, "hip:mi300", rebuild=True)
    finally:
        hip_codegen.TUNING["top_cache"] = saved
    program = type(hip)._gt_program_
    if program.plan.top_cache:
        assert any(k.top_cache is not None for k in program.kernels) and "_tc3(const gt_args a)" in program.source, text
    assert _lib.rtc_compile(program.source, f"two_sweep_{seed}.hip", ["-DGT4MI_UNIT_I_STRIDE=1", "-DGT4MI_NO_ALIAS=1"])[:4] == b"\x7fELF"


def test_most_two_sweep_programs_qualify(tmp_path):
    n = sum(bool(type(_two_sweep(seed, tmp_path, "hip:mi300")[0])._gt_program_.plan.top_cache) for seed in TWO_SWEEP_SEEDS[:30])
    assert n >= 20, f"only {n} of 30 random two-sweep programs are served by the top-of-column cache"


@pytest.mark.gpu
@pytest.mark.parametrize("seed", TWO_SWEEP_SEEDS)
def test_two_sweep_programs_match_the_oracle(seed, tmp_path):
    """GPU: random Thomas-like programs with shallow, seed-dependent cache depths on domains around the smallest one the
    `_tc` variant accepts, and with the default depths on a deep domain; every field bit for bit."""
    import random

    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian.backend import hip_codegen

    rnd = random.Random(seed)
    ref, scalars, text = _two_sweep(seed, tmp_path, "numpy")
    for depths, levels in (((rnd.randint(0, 6), rnd.randint(0, 6)), None), (None, rnd.choice([64, 97, 130, 161]))):
        saved = hip_codegen.TUNING["top_cache"]
        if depths is not None:
            hip_codegen.TUNING["top_cache"] = (depths[0], depths[1] * 8 * 3 * 256, 64)
        try:
            hip, _, _ = _two_sweep(seed, tmp_path, "hip:mi300", rebuild=True)
        finally:
            hip_codegen.TUNING["top_cache"] = saved
        kern = type(hip)._gt_program_.kernels[0]
        k_values = [levels] if levels else sorted({max(ref.domain_info.min_sequential_axis_size, k) for k in
                                                   ((kern.top_cache[-1][2] if kern.top_cache else 8) + d for d in (-1, 0, 1, 7))})
        for nk in k_values:
            domain = (66, 3, nk)
            arrays, origins = zoo.make_inputs(ref, domain, seed)
            expect = {k: v.copy() for k, v in arrays.items()}
            ref(**expect, **scalars, origin=origins, domain=domain)
            dev = {k: gt_storage.from_array(v, dtype=v.dtype, backend="hip:mi300", aligned_index=origins[k]) for k, v in arrays.items()}
            hip(**dev, **scalars, origin=origins, domain=domain)
            for k in arrays:
                np.testing.assert_array_equal(dev[k].get(), expect[k],
                                              err_msg=f"seed {seed} depths {depths} {domain} (cache {kern.top_cache}), field {k}\n{text}")


# ---- chains of horizontally offset temporaries: the strip kernel that shares them between lanes (`_vecs`) -----------
SHARED_SEEDS = list(range(_FIRST, _FIRST + (_N or 60)))


def _shared(seed, tmp_path, backend, **opts):
    import oracle.numpy_backend  # noqa: F401 - registers backend "numpy"
    from gt4py_amd.cartesian import gtscript

    defn, scalars, text = fuzz_stencils.make_shared_temporaries_stencil(seed, tmp_path)
    return gtscript.stencil(backend=backend, definition=defn, **opts), scalars, text


@pytest.mark.parametrize("seed", SHARED_SEEDS[::3])
def test_shared_temporaries_programs_compile(seed, tmp_path):
    """CPU: most random chains of offset temporaries get a `_vecs` kernel, and it compiles for gfx950 (the fuzzer found a
    compiler bug here: a float shifted between lanes and widened next made the DPP-combine pass emit v_cvt_f64_f32_dpp,
    which the target cannot encode -- hence the opaque shift)."""
    from gt4py_amd import _lib

    hip, _, text = _shared(seed, tmp_path, "hip:mi300")
    program = type(hip)._gt_program_
    if any(k.shared_halo for k in program.kernels):
        assert "_vecs(const gt_args a)" in program.source and "gt_shift<" in program.source, text
    assert _lib.rtc_compile(program.source, f"shared_{seed}.hip", ["-DGT4MI_UNIT_I_STRIDE=1", "-DGT4MI_NO_ALIAS=1"])[:4] == b"\x7fELF"


def test_most_shared_temporaries_programs_qualify(tmp_path):
    n = sum(any(k.shared_halo for k in type(_shared(seed, tmp_path, "hip:mi300")[0])._gt_program_.kernels) for seed in SHARED_SEEDS[:30])
    assert n >= 15, f"only {n} of 30 random programs with offset temporaries get the strip kernel that shares them"


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SHARED_SEEDS)
def test_shared_temporaries_programs_match_the_oracle(seed, tmp_path):
    """GPU: the same programs on domains of one, two and three waves in I with whole and partial 5-row strips; every
    field bit for bit against the oracle."""
    import gt4py_amd.storage as gt_storage

    ref, scalars, text = _shared(seed, tmp_path, "numpy")
    hip, _, _ = _shared(seed, tmp_path, "hip:mi300")
    for domain in ((130, 11, 2), (64, 5, 3), (300 + seed % 7, 8, 1)):
        domain = domain[:2] + (max(domain[2], ref.domain_info.min_sequential_axis_size),)
        arrays, origins = zoo.make_inputs(ref, domain, seed)
        expect = {k: v.copy() for k, v in arrays.items()}
        ref(**expect, **scalars, origin=origins, domain=domain)
        dev = {k: gt_storage.from_array(v, dtype=v.dtype, backend="hip:mi300", aligned_index=origins[k]) for k, v in arrays.items()}
        hip(**dev, **scalars, origin=origins, domain=domain)
        for k in arrays:
            np.testing.assert_array_equal(dev[k].get(), expect[k], err_msg=f"seed {seed} {domain}, field {k}\n{text}")


@pytest.mark.parametrize("seed", SHARED_SEEDS)
def test_shared_temporaries_rewritten_ir_matches_original_under_the_oracle(seed, tmp_path):
    """CPU: what the planner makes of these programs -- one temporary per interval block, conditionally assigned
    temporaries substituted as selects, everything inlined into one stage -- evaluated by the oracle against the
    original program, every field bit for bit."""
    import oracle.numpy_backend as oracle_backend
    from gt4py_amd.cartesian import analysis

    ref, scalars, text = _shared(seed, tmp_path, "numpy")
    hip, _, _ = _shared(seed, tmp_path, "hip:mi300")
    program = type(hip)._gt_program_
    domain = (9, 7, max(3, ref.domain_info.min_sequential_axis_size))
    arrays, origins = zoo.make_inputs(ref, domain, seed)
    expect = {k: v.copy() for k, v in arrays.items()}
    ref(**expect, **scalars, origin=origins, domain=domain)
    got = {k: v.copy() for k, v in arrays.items()}
    rewritten = program.plan.stencil
    oracle_backend.run_stencil(rewritten, analysis.compute_extents(rewritten), domain, origins, got, scalars)
    for k in arrays:
        np.testing.assert_array_equal(got[k], expect[k], err_msg=f"seed {seed}, field {k}\n{text}")


# ---- typed programs: integers, bools, casts and mixed kinds (the expression layer of the code generator) ----------------------------
TYPED_SEEDS = list(range(_FIRST, _FIRST + (_N or 120)))


def _typed(seed, tmp_path, backend):
    import oracle.numpy_backend  # noqa: F401 - registers backend "numpy"
    from gt4py_amd.cartesian import gtscript

    defn, scalars, text = fuzz_stencils.make_typed_stencil(seed, tmp_path)
    return gtscript.stencil(backend=backend, definition=defn), scalars, text, defn


@pytest.mark.parametrize("seed", TYPED_SEEDS)
def test_typed_rewritten_ir_matches_original_under_the_oracle(seed, tmp_path):
    """CPU: what the planner makes of a typed program (inlined temporaries keep their casts, masks stay bools) evaluates to the
    original program's bits under the numpy oracle; every sixth program is compiled for gfx950."""
    import oracle.numpy_backend as oracle_backend
    from gt4py_amd import _lib
    from gt4py_amd.cartesian import analysis
    from test_oracle_independent import assert_same_bits, defined_casts_only

    ref, scalars, text, _ = _typed(seed, tmp_path, "numpy")
    hip, _, _, _ = _typed(seed, tmp_path, "hip:mi300")
    program = type(hip)._gt_program_
    assert ref.field_info == hip.field_info
    for domain in ((9, 7, 5), (5, 4, 3)):
        arrays, origins = zoo.make_typed_inputs(ref, domain, seed)
        expect = {k: v.copy() for k, v in arrays.items()}
        got = {k: v.copy() for k, v in arrays.items()}
        rewritten = program.plan.stencil
        with defined_casts_only():
            ref(**expect, **scalars, origin=origins, domain=domain)
            oracle_backend.run_stencil(rewritten, analysis.compute_extents(rewritten), domain, origins, got, scalars)
        for k in arrays:
            assert_same_bits(got[k], expect[k], f"seed {seed} {domain}, field {k}\n{text}")
    if seed % 6 == 0:
        assert _lib.rtc_compile(program.source, f"typed_{seed}.hip", ["-DGT4MI_UNIT_I_STRIDE=1", "-DGT4MI_NO_ALIAS=1"])[:4] == b"\x7fELF"


def _census_interpreter():
    """The independent interpreter with a tally of the constructs it EVALUATES (on at least one point of a box), by the dtypes
    and values the operands have there."""
    import ast

    from oracle import gtscript_interp as gi

    class Census(gi.Interpreter):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.seen, self._quiet = set(), 0

        def _eval(self, e, box, env, shift):
            out = super()._eval(e, box, env, shift)
            if not self._quiet and isinstance(e, (ast.BinOp, ast.Compare, ast.BoolOp, ast.UnaryOp, ast.Call)):
                self._quiet += 1
                try:
                    self._note(e, [np.asarray(super(Census, self)._eval(x, box, env, shift)) for x in self._operands(e)])
                finally:
                    self._quiet -= 1
            return out

        @staticmethod
        def _operands(e):
            if isinstance(e, ast.BinOp):
                return [e.left, e.right]
            if isinstance(e, ast.Compare):
                return [e.left, e.comparators[0]]
            if isinstance(e, ast.UnaryOp) and not isinstance(e.operand, ast.Constant):
                return [e.operand]
            if isinstance(e, ast.Call) and getattr(e.func, "id", None) == "abs":
                return list(e.args)
            return []

        def _note(self, e, v):
            kinds = [x.dtype.kind for x in v]
            if isinstance(e, ast.BoolOp) or (isinstance(e, ast.UnaryOp) and isinstance(e.op, ast.Not)):
                self.seen.add("and / or / not")
            elif isinstance(e, ast.Compare):
                if kinds[0] != kinds[1]:
                    self.seen.add("mixed-kind comparison")
            elif isinstance(e, ast.BinOp):
                integers = all(k in "ib" for k in kinds)
                if isinstance(e.op, ast.Mod):
                    t = gi._ufunc_targets(np.remainder, [x.dtype for x in v])[0]
                    if (v[1] < 0).any():
                        self.seen.add("int % negative" if t.kind == "i" else "float % negative")
                    if t.kind == "i" and (v[1] == 0).any():
                        self.seen.add("int % 0")
                elif isinstance(e.op, ast.Pow):
                    if integers:
                        self.seen.add("int ** int")
                        self._overflow(np.result_type(*[x.dtype for x in v]), v[0].astype(object) ** np.maximum(v[1], 0).astype(object))
                    elif kinds == ["f", "i"]:
                        self.seen.add("float ** int")
                elif isinstance(e.op, ast.Div):
                    if integers:
                        self.seen.add("int / int")
                elif integers:
                    uf = {ast.Add: np.add, ast.Sub: np.subtract, ast.Mult: np.multiply}[type(e.op)]
                    self._overflow(gi._ufunc_targets(uf, [x.dtype for x in v])[0], uf(v[0].astype(object), v[1].astype(object)))
            elif v and kinds[0] == "i" and (v[0] == np.iinfo(v[0].dtype).min).any():  # unary minus, abs
                self.seen.add("abs / - of iinfo.min")

        def _overflow(self, dtype, exact):
            """`exact`: the node's value in Python integers; it overflows when that leaves the dtype the node computes in."""
            if dtype in (np.dtype("int32"), np.dtype("int64")):
                lim = np.iinfo(dtype)
                if any(int(x) < lim.min or int(x) > lim.max for x in np.asarray(exact, dtype=object).ravel()):
                    self.seen.add("int32 / int64 overflow")

        def _assign(self, target, value_ast, box, mask, value):
            if value is None:
                value = self._eval(value_ast, box, {}, (0, 0, 0))
            super()._assign(target, value_ast, box, mask, value)
            stored, v = self.flds[self._target(target)[0]].dtype, np.asarray(value)
            if v.dtype.kind == "f" and stored.kind == "i":
                self.seen.add("float -> int store")
            if v.dtype.kind == "i" and stored in (np.dtype("int8"), np.dtype("int16")) and (v.astype(stored) != v).any():
                self.seen.add("int -> int8 / int16 store that wraps")

    return Census


CENSUS = ("int % negative", "float % negative", "int % 0", "int ** int", "float ** int", "int / int", "mixed-kind comparison",
          "and / or / not", "float -> int store", "int -> int8 / int16 store that wraps", "int32 / int64 overflow", "abs / - of iinfo.min")


def test_the_typed_corpus_evaluates_every_construct_it_is_meant_for(tmp_path):
    """Census over the typed corpus on (9, 7, 5), printed and asserted: each construct is EVALUATED in at least 5 programs."""
    from test_oracle_independent import defined_casts_only

    Census = _census_interpreter()
    count = {c: 0 for c in CENSUS}
    for seed in TYPED_SEEDS:
        ref, scalars, text, defn = _typed(seed, tmp_path, "numpy")
        arrays, origins = zoo.make_typed_inputs(ref, (9, 7, 5), seed)
        it = Census(defn)
        with defined_casts_only():
            it({k: (v, origins[k]) for k, v in arrays.items()}, scalars, (9, 7, 5))
        assert it.seen <= set(CENSUS)
        for c in it.seen:
            count[c] += 1
    print(f"of {len(TYPED_SEEDS)} typed programs: " + ", ".join(f"{c}: {n}" for c, n in count.items()))
    assert all(n >= 5 for n in count.values()), count


def test_kernel_kinds_the_typed_corpus_reaches_with_non_float_fields(tmp_path):
    """Every typed program has integer (and often bool) fields.  Counted over the corpus: programs that get a point-per-thread
    kernel, a `_vec` strip kernel, a `_vecs` strip kernel, a column kernel -- all four must occur -- and a `_tc` kernel, which never
    does, for two reasons: stage_planner's top-of-column cache takes a column stage of FORWARD nests followed by BACKWARD nests
    (`n_first == 0 or n_first == len(stage.nests)` -> no cache), and the generator emits ONE sweep per program; and its rule
    `np.dtype(d.dtype).itemsize not in (4, 8)` keeps bool, int8 and int16 fields out of the cache where a two-sweep program has
    them (tests/test_stencil_refusals.py-style refusal, here a silent `continue`).  The strip kernels are offered only programs
    whose every I-J-K array has 4- or 8-byte items (hip_codegen._vector_width: `sizes <= {4, 8}`; _shared_form: a shifted
    temporary of another size -> None), so `gt_shift` never sees a 1- or 2-byte type: asserted here on the emitted source."""
    import re

    count = {"point": 0, "_vec": 0, "_vecs": 0, "column": 0, "_tc": 0}
    for seed in TYPED_SEEDS:
        hip, _, text, _ = _typed(seed, tmp_path, "hip:mi300")
        program = type(hip)._gt_program_
        assert any(np.dtype(f.dtype).kind != "f" for f in program.plan.stencil.fields)
        ks = program.kernels
        count["point"] += any(k.mapping == "ijk" and not k.vec and not k.shared_halo for k in ks)
        count["_vec"] += any(k.vec for k in ks)
        count["_vecs"] += any(k.shared_halo for k in ks)
        count["column"] += any(k.mapping == "column" for k in ks)
        count["_tc"] += any(k.top_cache for k in ks)
        for ct in re.findall(r"gt_shift<([a-z ]+),", program.source):
            assert ct in ("int", "long long", "float", "double"), (ct, text)
    print(f"of {len(TYPED_SEEDS)} typed programs: " + ", ".join(f"{k}: {n}" for k, n in count.items()))
    assert count["point"] and count["_vec"] and count["_vecs"] and count["column"], count
    assert count["_tc"] == 0, count


# ---- directed tables: the anchor of the typed fuzzer (expected values are plain numpy, nothing from either oracle) ---------------------
TABLE_DOMAIN = (66, 3, 2)
_OPS = ("add", "sub", "mul", "mod", "neg", "ab", "pw", "mn", "mx")
_CMPS = (("gt", ">"), ("lt", "<"), ("ge", ">="), ("le", "<="), ("eq", "=="), ("ne", "!="))


def _load(text, name, tmp_path):
    import importlib.util

    path = tmp_path / f"{name}.py"
    path.write_text(fuzz_stencils.HEADER.format(seed="directed table") + text)
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return getattr(module, name)


def _along_i(values, dtype):
    """`values` repeated along I over TABLE_DOMAIN, the same on every row and level."""
    line = np.resize(np.asarray(values, dtype=dtype), TABLE_DOMAIN[0])
    return np.ascontiguousarray(np.broadcast_to(line[:, None, None], TABLE_DOMAIN))


def _run_table(defn, arrays):
    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript

    hip = gtscript.stencil(backend="hip:mi300", definition=defn)
    dev = {k: gt_storage.from_array(v, dtype=v.dtype, backend="hip:mi300", aligned_index=(0, 0, 0)) for k, v in arrays.items()}
    hip(**dev, origin=(0, 0, 0), domain=TABLE_DOMAIN)
    return {k: v.get() for k, v in dev.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["int8", "int16", "int32", "int64"])
def test_integer_operator_table(name, tmp_path):
    """All pairs of {min, min + 1, -7, -1, 0, 1, 7, max} of an integer dtype through every operator, against numpy's own wrapping
    arithmetic.  `a / b` is float32 for every integer dtype: the reference's upcasting rule takes the lowest-ranking loop of
    np.true_divide both operands fit, `ff->f`.  `a ** (abs(b) % 4)` is computed in int64 (the literal 4) and narrowed by the store."""
    from test_oracle_independent import assert_same_bits

    dt = np.dtype(name)
    lim = np.iinfo(dt)
    vals = [lim.min, lim.min + 1, -7, -1, 0, 1, 7, lim.max]
    a = _along_i([x for x in vals for _ in vals], dt)
    b = _along_i([y for _ in vals for y in vals], dt)
    fields = [f"{o}: Field[np.{name}]" for o in _OPS] + ["div: Field[np.float32]"] + [f"{c}: Field[np.bool_]" for c, _ in _CMPS]
    body = ["add = a + b", "sub = a - b", "mul = a * b", "mod = a % b", "div = a / b", "neg = -a", "ab = abs(a)",
            "pw = a ** (abs(b) % 4)", "mn = min(a, b)", "mx = max(a, b)"] + [f"{c} = a {op} b" for c, op in _CMPS]
    text = (f"\n\ndef table_{name}(a: Field[np.{name}], b: Field[np.{name}], {', '.join(fields)}):\n"
            "    with computation(PARALLEL), interval(...):\n" + "".join(f"        {ln}\n" for ln in body))
    arrays = {"a": a, "b": b, "div": np.zeros(TABLE_DOMAIN, np.float32)}
    arrays.update({o: np.zeros(TABLE_DOMAIN, dt) for o in _OPS})
    arrays.update({c: np.zeros(TABLE_DOMAIN, np.bool_) for c, _ in _CMPS})
    with np.errstate(all="ignore"):
        want = {"a": a, "b": b, "add": a + b, "sub": a - b, "mul": a * b, "mod": np.remainder(a, b),
                "div": a.astype(np.float32) / b.astype(np.float32), "neg": np.negative(a), "ab": np.abs(a),
                "pw": np.power(a.astype(np.int64), np.remainder(np.abs(b).astype(np.int64), np.int64(4))).astype(dt),
                "mn": np.minimum(a, b), "mx": np.maximum(a, b), "gt": a > b, "lt": a < b, "ge": a >= b, "le": a <= b, "eq": a == b, "ne": a != b}
    got = _run_table(_load(text, f"table_{name}", tmp_path), arrays)
    for k in want:
        assert_same_bits(got[k], want[k], f"{name}: {k}")


_CAST_DTYPES = ("bool_", "int8", "int16", "int32", "int64", "float32", "float64")


@pytest.mark.gpu
def test_cast_table(tmp_path):
    """Every (source, destination) dtype pair as a narrowing / widening store, and the four cast functions, against `astype`.
    Sources hold only values whose conversion numpy defines for EVERY destination (finite floats below 100 in magnitude, with
    -0.0 and halves; integers up to the edges of their dtype, 300, 16777217 and 2**53 + 1 among them); NaN, infinities and
    huge floats go to bool and to the float dtypes only."""
    from test_oracle_independent import assert_same_bits

    small = [-0.0, 0.0, 0.5, -0.5, 1.5, -1.5, 2.5, 99.75, -99.25, 1.0, -1.0, 0.1, 127.0, -128.0, 1e-30]
    wild = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 1e300, -1e300, 1e-300, 3.4028235e38, 16777217.0, 0.1]
    ints = {"int8": [-128, -127, -1, 0, 1, 127], "int16": [-32768, -129, -1, 0, 1, 128, 255, 256, 300, 32767],
            "int32": [-2**31, -32769, -129, 0, 1, 300, 65536, 16777217, 2**31 - 1],
            "int64": [-2**63, -2**31 - 1, -129, 0, 1, 300, 2**32, 16777217, 2**53 + 1, 2**63 - 1]}
    src = {"s_bool_": _along_i([True, False, True], np.bool_)}
    src.update({f"s_{n}": _along_i(v, n) for n, v in ints.items()})
    src.update({"s_float32": _along_i(small, np.float32), "s_float64": _along_i(small, np.float64)})
    wild_src = {"w_float32": _along_i(wild, np.float32), "w_float64": _along_i(wild, np.float64)}
    outs, body, want = {}, [], {}
    with np.errstate(all="ignore"):
        for s in _CAST_DTYPES:
            for d in _CAST_DTYPES:
                outs[f"o_{s}_{d}"] = np.dtype(d)
                body.append(f"o_{s}_{d} = s_{s}")
                want[f"o_{s}_{d}"] = src[f"s_{s}"].astype(d)
            for d in ("int32", "int64", "float32", "float64"):  # the cast functions, then a store of the same dtype
                outs[f"c_{s}_{d}"] = np.dtype(d)
                body.append(f"c_{s}_{d} = {d}(s_{s})")
                want[f"c_{s}_{d}"] = src[f"s_{s}"].astype(d)
        for s in ("float32", "float64"):
            for d in ("bool_", "float32", "float64"):
                outs[f"x_{s}_{d}"] = np.dtype(d)
                body.append(f"x_{s}_{d} = w_{s}")
                want[f"x_{s}_{d}"] = wild_src[f"w_{s}"].astype(d)
    assert want["o_int16_int8"][8, 0, 0] == 44 and want["o_int64_float64"][8, 0, 0] == 2.0**53  # 300 wraps, 2**53 + 1 rounds
    assert want["o_int32_float32"][7, 0, 0] == 16777216.0 and want["x_float64_bool_"][0, 0, 0] and not want["x_float64_bool_"][4, 0, 0]
    inputs = {**src, **wild_src}
    sig = [f"{k}: Field[np.{v.dtype.name if v.dtype != np.bool_ else 'bool_'}]" for k, v in inputs.items()]
    sig += [f"{k}: Field[np.{d.name if d != np.bool_ else 'bool_'}]" for k, d in outs.items()]
    text = (f"\n\ndef cast_table({', '.join(sig)}):\n    with computation(PARALLEL), interval(...):\n"
            + "".join(f"        {ln}\n" for ln in body))
    arrays = {**inputs, **{k: np.zeros(TABLE_DOMAIN, d) for k, d in outs.items()}}
    got = _run_table(_load(text, "cast_table", tmp_path), arrays)
    for k, v in {**inputs, **want}.items():
        assert_same_bits(got[k], v, f"cast table: {k}")
