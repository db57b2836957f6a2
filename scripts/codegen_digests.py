#!/usr/bin/env python
"""One line per generated program: name, sha256 of the HIP source, the kernels' launch records, the inexact calls.

Needs no GPU.  Run it on two trees (PYTHONPATH=<tree>:<tree>/tests) and `diff` the outputs: an emitter refactor
that is meant to leave the generated kernels alone must leave every line alone.  Corpus: tests/stencil_zoo.py at the
defaults, its two-sweep programs at two shallow top-of-column cache settings (every range kind: memory, LDS,
registers), every suite of tests/reference_suites.py, 200 random stencils and 60 random two-sweep programs of
tests/fuzz_stencils.py (the latter also at the shallow seed-dependent depths of tests/test_fuzz_codegen.py).
"""

import dataclasses
import hashlib
import pathlib
import random
import sys
import tempfile

HERE = pathlib.Path(__file__).resolve().parent
for extra in (HERE.parent, HERE.parent / "tests"):  # appended: a tree named in PYTHONPATH wins
    if str(extra) not in sys.path:
        sys.path.append(str(extra))

import fuzz_stencils  # noqa: E402
import reference_suites  # noqa: E402
import stencil_zoo  # noqa: E402

from gt4py_amd.cartesian import gtscript  # noqa: E402
from gt4py_amd.cartesian.backend import hip_codegen  # noqa: E402

TWO_SWEEP_ZOO = ("tridiagonal_solver", "vertical_advection_dycore", "two_sweep_three_carried")
TOP_CACHE_SETTINGS = ((3, 4 * 8 * 3 * 256), (0, 2 * 8 * 3 * 256, 64))


def _kernel_repr(kern) -> str:
    # (without the K levels / J rows per thread that older trees recorded: always 1)
    items = [(f.name, getattr(kern, f.name)) for f in dataclasses.fields(kern) if not f.name.endswith("_per_thread")]
    return "KernelSource(" + ", ".join(f"{n}={v!r}" for n, v in items) + ")"


def line(label: str, **stencil_args) -> str:
    stencil_args.setdefault("use_kernel_library", False)  # the generated program, also where the kernel library would serve
    st = gtscript.stencil(backend="hip:mi300", rebuild=True, **stencil_args)
    program = type(st)._gt_program_
    digest = hashlib.sha256(program.source.encode()).hexdigest()
    return f"{label} {digest} [{', '.join(_kernel_repr(k) for k in program.kernels)}] {sorted(program.inexact_calls)}"


def with_top_cache(setting, label: str, **stencil_args) -> str:
    saved = hip_codegen.TUNING["top_cache"]
    hip_codegen.TUNING["top_cache"] = setting
    try:
        return line(label, **stencil_args)
    finally:
        hip_codegen.TUNING["top_cache"] = saved


def main() -> None:
    out = []
    for name, (defn, externals, _, opts) in stencil_zoo.ZOO.items():
        out.append(line(f"zoo:{name}", definition=defn, externals=externals, **opts))
    for name in TWO_SWEEP_ZOO:
        defn, externals, _, opts = stencil_zoo.ZOO[name]
        for setting in TOP_CACHE_SETTINGS:
            out.append(with_top_cache(setting, f"zoo:{name}:top_cache={setting}", definition=defn, externals=externals, **opts))
    for name, suite in reference_suites.SUITES.items():
        for n, ext in enumerate(suite.externals):
            out.append(line(f"suite:{name}:{n}", definition=suite.definition, externals=ext))
    with tempfile.TemporaryDirectory() as tmp:
        for seed in range(200):
            defn, _, _ = fuzz_stencils.make_stencil(seed, tmp)
            out.append(line(f"fuzz:{seed}", definition=defn))
        for seed in range(60):
            defn, _, _ = fuzz_stencils.make_two_sweep_stencil(seed, tmp)
            out.append(line(f"two_sweep:{seed}", definition=defn))
            rnd = random.Random(seed)  # the depths tests/test_fuzz_codegen.py draws for this seed
            depths = (rnd.randint(0, 6), rnd.randint(0, 6))
            setting = (depths[0], depths[1] * 8 * 3 * 256, 64)
            out.append(with_top_cache(setting, f"two_sweep:{seed}:top_cache={setting}", definition=defn))
    print("\n".join(out))


if __name__ == "__main__":
    main()
