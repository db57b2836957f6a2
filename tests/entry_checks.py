"""What the CPU test of a utility entry starts from: native descriptors over made-up addresses, a DeviceArray around host memory,
the declaration check (header against binding against library), the kernels' lines of the resource log, and the pretence that
host memory is on the device.  A plain module, imported like ``gpu_util``; what a utility's test is about stays in its file."""

import ctypes
import gc
import pathlib
import re

import pytest

from gt4py_amd import _lib

ROOT = pathlib.Path(__file__).resolve().parent.parent
INV, OOB, UNS = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_OUT_OF_BOUNDS, _lib.ERR_UNSUPPORTED


# ---- descriptors ---------------------------------------------------------------------------------------------------------------
def field(ptr, shape, strides=None, origin=(1, 1, 0), itemsize=8, layout="ifirst"):
    """A gt4mi_field at a made-up address; without ``strides``, packed in ``layout`` (the axis named first is contiguous)."""
    if strides is None:
        ni, nj, nk = shape
        strides = {"ifirst": (1, ni, ni * nj), "kfirst": (nj * nk, nk, 1), "jfirst": (nj, 1, ni * nj)}[layout]
        strides = tuple(s * itemsize for s in strides)
    return _lib.Field.make(ptr, shape, strides, origin)


def line(ptr, n, axis, itemsize=8):
    """A 1-d field of ``n`` items along ``axis``: extent 1 and stride 0 on the other two."""
    shape, strides = [1, 1, 1], [0, 0, 0]
    shape[axis], strides[axis] = n, itemsize
    return _lib.Field.make(ptr, shape, strides, (0, 0, 0))


def plane(ptr, shape_ij, origin, itemsize=8):
    """An IJ field: one level, stride 0 along K."""
    ni, nj = shape_ij
    return _lib.Field.make(ptr, (ni, nj, 1), (itemsize, ni * itemsize, 0), origin)


def as_arg(f):
    """One descriptor goes by reference; an array of them, an address or None goes as it is."""
    return ctypes.byref(f) if isinstance(f, ctypes.Structure) else f


def int64s(values):
    return None if values is None else (ctypes.c_int64 * len(values))(*values)


def table(fields):
    fields = list(fields)
    return (_lib.Field * len(fields))(*fields)


def call(entry, *args, outs=()):
    """``entry(*args, &out...)``: every sentinel of ``outs`` (an int stands for a C int) goes by reference behind ``args``.
    Returns ``(rc, message, *out values)``."""
    lib = _lib.load()
    outs = [o if isinstance(o, ctypes._SimpleCData) else ctypes.c_int(o) for o in outs]
    rc = getattr(lib, entry)(*args, *map(ctypes.byref, outs))
    return (rc, lib.gt4mi_last_error(), *(o.value for o in outs))


def host_field(shape, dtype="float64"):
    """A DeviceArray around HOST memory: enough for every argument check (they need no device); a call that passed them all
    is refused last, for not being on the device."""
    import torch

    from gt4py_amd.storage.device_array import DeviceArray, torch_dtype

    return DeviceArray(torch.zeros(shape, dtype=torch_dtype(dtype)))


def on_device(monkeypatch):
    """Pretend host memory is on the device: a frozen call's device check passes, the launch is never reached."""
    import torch

    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: None)


def refuses_a_dead_array(frozen):
    """After the test deleted an array ``frozen`` was bound to: the call finds the dead weak reference first."""
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        frozen()


# ---- the declaration -----------------------------------------------------------------------------------------------------------
_I64P = ctypes.POINTER(ctypes.c_int64)
CTYPE_OF = {  # declared parameter type (an array parameter is a pointer) -> what the binding must declare
    "int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
    "void*": ctypes.c_void_p, "const void*": ctypes.c_void_p,
    "int*": ctypes.POINTER(ctypes.c_int), "int64_t*": _I64P, "const int64_t*": _I64P,
    "const gt4mi_field*": ctypes.POINTER(_lib.Field), "const gt4mi_overlap_axis*": ctypes.POINTER(_lib.OverlapAxis),
}


def derived_argtypes(params):
    """The ctypes of a header parameter list through CTYPE_OF; a type that is not in the table raises."""
    types = []
    for p in params:
        ctype, array = re.fullmatch(r"(.*?)\s*\w+(\[\d+\])?", p).groups()
        types.append(CTYPE_OF[ctype + ("*" if array else "")])
    return types


def check_binding(entry, params, prefix=None, constants=(), phrases=(), argtypes=None):
    """The header declares ``int entry(params)`` at ABI 8, ``_lib`` binds it with the matching ctypes (``argtypes`` where the
    binding passes a typed pointer as an address, else derived from ``params``), exports it and the library has it; the comment
    block in front of the declaration holds every one of ``phrases``; the ``GT4MI_<prefix>_*`` enumerators named in
    ``constants`` have ``_lib``'s values."""
    text = (ROOT / "include" / "gt4py_amd.h").read_text()
    assert re.search(r"#define GT4MI_ABI_VERSION 8\b", text) and _lib.GT4MI_ABI_VERSION == 8
    assert _lib.load().gt4mi_abi_version() == 8
    decl = re.search(rf"int {entry}\((.*?)\);", text, re.S).group(1)
    assert [" ".join(p.split()) for p in decl.split(",")] == params
    fn = getattr(_lib.load(), entry)
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == (derived_argtypes(params) if argtypes is None else argtypes)
    assert entry in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), entry)
    comment = text[: text.index(f"int {entry}(")].rsplit("/* ----", 1)[1]
    for phrase in phrases:
        assert phrase in comment, phrase
    for name in constants:
        value = int(re.search(rf"GT4MI_{prefix}_{name} = (\d+)", text).group(1))
        assert getattr(_lib, f"{prefix}_{name}") == value, name


# ---- the resource log ----------------------------------------------------------------------------------------------------------
def kernel_resources(pattern):
    """``(name, scratch bytes per lane, waves per SIMD, LDS bytes per block)`` of every kernel whose mangled name holds
    ``pattern``, from the log the build writes next to the library."""
    log = _lib.LIB_PATH.with_name("libgt4py_amd.resources.log")
    assert log.exists(), "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    found = re.findall(rf"remark: Function Name: (\S*{pattern}\S*).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                       r"Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", log.read_text(), re.S)
    return [(name, int(scratch), int(waves), int(lds)) for name, scratch, waves, lds in found]
