"""ORACLE (test infrastructure): ctypes wrapper + build recipe for oracle/cpu_ifirst.c.

``build()`` compiles the C restatement into ``oracle/_build/libcpu_ifirst.so`` (git-ignored; it
travels to the GPU box with the snapshot).  Only tests/, ``__graft_entry__`` and bench.py's
cpu_baseline leg use this module.
"""

from __future__ import annotations

import ctypes
import os
import pathlib
import subprocess
from typing import Optional, Sequence

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "cpu_ifirst.c"
BUILD_DIR = HERE / "_build"
LIB = BUILD_DIR / "libcpu_ifirst.so"

_lib: Optional[ctypes.CDLL] = None


def build(march: str = "x86-64-v3", out: Optional[pathlib.Path] = None, quiet: bool = True) -> pathlib.Path:
    """gcc -O3 -fopenmp -ffp-contract=off (no FMA contraction: bit parity with numpy)."""
    out = pathlib.Path(out) if out is not None else LIB
    out.parent.mkdir(parents=True, exist_ok=True)
    cmd = ["gcc", "-O3", f"-march={march}", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-shared",
           "-fPIC", "-o", str(out), str(SRC)]
    subprocess.run(cmd, check=True, capture_output=quiet)
    return out


def available() -> bool:
    return LIB.exists()


def load(path: Optional[pathlib.Path] = None) -> ctypes.CDLL:
    global _lib
    if path is None and _lib is not None:
        return _lib
    lib = ctypes.CDLL(str(path or LIB))
    i64, dp, fp, cint = ctypes.c_int64, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float), ctypes.c_int
    lib.oracle_set_threads.argtypes = [cint]
    lib.oracle_max_threads.restype = cint
    lib.oracle_lap5_f64.argtypes = [dp, i64, i64, i64, dp, i64, i64, i64, i64, i64, i64]
    for name, p in (("oracle_lap5_f64_variant", dp), ("oracle_lap5_f32", fp), ("oracle_lap5_f32_lit32", fp)):
        getattr(lib, name).argtypes = [p, i64, i64, i64, p, i64, i64, i64, i64, i64, i64, cint]
        getattr(lib, name).restype = cint
    for name, p in (("oracle_hdiff_f64", dp), ("oracle_hdiff_f32", fp), ("oracle_hdiff_f32_w32", fp), ("oracle_hdiff_f32_w32_p64", fp)):
        getattr(lib, name).argtypes = [p, i64, i64, i64, p, i64, i64, i64, p, i64, i64, i64, ctypes.c_double, i64, i64, i64, cint]
    lib.oracle_tridiag_f64.argtypes = [dp, dp, dp, dp, dp, i64, i64, i64, i64, i64, i64]
    lib.oracle_tridiag_f32.argtypes = [fp, fp, fp, fp, fp, i64, i64, i64, i64, i64, i64]
    if path is None:
        _lib = lib
    return lib


def _ptr(a: np.ndarray, origin: Sequence[int]):
    isz = a.dtype.itemsize
    assert a.dtype in (np.float64, np.float32), a.dtype
    assert all(s % isz == 0 for s in a.strides)
    off = sum(int(o) * s for o, s in zip(origin, a.strides))
    ctype = ctypes.c_double if a.dtype == np.float64 else ctypes.c_float
    return ctypes.cast(a.ctypes.data + off, ctypes.POINTER(ctype)), [s // isz for s in a.strides]


def _setup(lib, threads):
    lib = lib or load()
    if threads:
        lib.oracle_set_threads(threads)
    return lib


def lap5_f64(inp, out, origin_inp, origin_out, domain, threads: int = 0, lib=None) -> None:
    lib = _setup(lib, threads)
    pi, si = _ptr(inp, origin_inp)
    po, so = _ptr(out, origin_out)
    lib.oracle_lap5_f64(pi, *si, po, *so, *map(int, domain))


def lap5(inp, out, origin_inp, origin_out, domain, variant: int = 0, literal32: bool = False, threads: int = 0, lib=None) -> None:
    """Every variant of csrc/lap5.hip.h:lap5_expr (0..3 = notebook, docs, suite, avg) for float64 and float32 fields;
    ``literal32``: the float literals are float32 (GT4MI_LAP_LITERAL_F32, float32 fields only)."""
    lib = _setup(lib, threads)
    assert inp.dtype == out.dtype
    if inp.dtype == np.float64:
        assert not literal32, "literal precision 32 applies to float32 fields only"
        fn = lib.oracle_lap5_f64_variant
    else:
        fn = lib.oracle_lap5_f32_lit32 if literal32 else lib.oracle_lap5_f32
    pi, si = _ptr(inp, origin_inp)
    po, so = _ptr(out, origin_out)
    if fn(pi, *si, po, *so, *map(int, domain), int(variant)) != 0:
        raise ValueError(f"unknown lap5 variant {variant}")


def hdiff(inp, out, coeff, origin_in, origin_out, origin_coeff, domain, limiter: bool = True, internal_f32: bool = False,
          coeff_f32: bool = False, threads: int = 0, lib=None) -> None:
    """Horizontal diffusion with the (W, PW) choice of csrc/hdiff.hip.h:hdiff_run: ``coeff`` is a field (an array) or a
    scalar; ``internal_f32`` = GT4MI_HDIFF_INTERNAL_F32 (literal_float_precision=32), ``coeff_f32`` = GT4MI_HDIFF_COEFF_F32
    (a float32 scalar: rounded through float first)."""
    lib = _setup(lib, threads)
    assert inp.dtype == out.dtype
    field = isinstance(coeff, np.ndarray) and coeff.ndim == 3
    cs = 0.0
    if field:
        assert coeff.dtype == inp.dtype
        pc, sc = _ptr(coeff, origin_coeff)
    else:
        pc, sc = None, [0, 0, 0]
        cs = float(np.float32(coeff)) if coeff_f32 else float(coeff)
    if inp.dtype == np.float64:
        assert not internal_f32, "float32 internals apply to float32 fields only"
        fn = lib.oracle_hdiff_f64
    elif not internal_f32:
        fn = lib.oracle_hdiff_f32
    elif field or coeff_f32:
        fn = lib.oracle_hdiff_f32_w32
    else:
        fn = lib.oracle_hdiff_f32_w32_p64
    pi, si = _ptr(inp, origin_in)
    po, so = _ptr(out, origin_out)
    fn(pi, *si, po, *so, pc, *sc, cs, *map(int, domain), int(limiter))


def tridiag(inf, diag, sup, rhs, out, domain, threads: int = 0, lib=None) -> None:
    """Thomas solve on identically laid out float64 or float32 fields (origin 0); ``sup`` and ``rhs`` are rewritten."""
    lib = _setup(lib, threads)
    arrs = (inf, diag, sup, rhs, out)
    assert len({tuple(a.strides) for a in arrs}) == 1, "tridiag oracle expects identically laid out fields"
    assert len({a.dtype for a in arrs}) == 1
    ptrs = [_ptr(a, (0, 0, 0)) for a in arrs]
    fn = lib.oracle_tridiag_f64 if inf.dtype == np.float64 else lib.oracle_tridiag_f32
    fn(*[p for p, _ in ptrs], *ptrs[0][1], *map(int, domain))


def tridiag_f64(inf, diag, sup, rhs, out, domain, threads: int = 0, lib=None) -> None:
    assert inf.dtype == np.float64
    tridiag(inf, diag, sup, rhs, out, domain, threads=threads, lib=lib)
