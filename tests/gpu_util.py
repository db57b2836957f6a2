"""Helpers for the GPU parity tests: device buffers with a chosen memory layout + C-ABI calls."""

from __future__ import annotations

import ctypes

import numpy as np
import torch

from device_layouts import geometry
from gt4py_amd import _lib

TORCH_DT = {np.dtype("float64"): torch.float64, np.dtype("float32"): torch.float32}


class DevArray:
    """A device copy of a numpy IJK array with a selectable layout.

    The geometry is tests/device_layouts.py's:
    layout "ifirst"  : I contiguous, rows padded so that element [align_index[0], j, k] is aligned to
                       256 bytes (what gt4py storages for gt:gpu / hip:mi300 look like)
    layout "ifirst_unaligned": I contiguous, rows padded to an odd pitch and base offset by one item
    layout "kfirst"  : C order of (I, J, K) -- K contiguous (numpy backend default)
    layout "jfirst"  : J contiguous
    """

    def __init__(self, host: np.ndarray, layout: str = "ifirst", align_index=(0, 0, 0)):
        assert host.ndim == 3
        self.host_shape = host.shape
        self.dtype = host.dtype
        numel, self.strides, offset = geometry(host.shape, layout, host.dtype.itemsize, align_index[0])
        self._flat = torch.empty(numel, dtype=TORCH_DT[host.dtype], device="cuda")  # (over-allocated: the aligned base is inside)
        self.offset = offset(self._flat.data_ptr())
        self._flat.fill_(float("nan"))
        self.view = torch.as_strided(self._flat, host.shape, self.strides, self.offset)
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(host)))

    @property
    def ptr(self) -> int:
        return self._flat.data_ptr() + self.offset * self.dtype.itemsize

    def field(self, origin) -> _lib.Field:
        bs = tuple(s * self.dtype.itemsize for s in self.strides)
        return _lib.Field.make(self.ptr, self.host_shape, bs, origin)

    def get(self) -> np.ndarray:
        torch.cuda.synchronize()
        return self.view.cpu().numpy()


def device(box, layout, halo, align_i=None):
    """A DevArray of the box inside `halo` ghost cells in I and J, NaN everywhere outside the box."""
    host = np.full((box.shape[0] + 2 * halo, box.shape[1] + 2 * halo, box.shape[2]), np.nan, dtype=box.dtype)
    host[halo: halo + box.shape[0], halo: halo + box.shape[1]] = box
    return DevArray(host, layout, align_index=(halo if align_i is None else align_i, 0, 0))


def wrap(dev):
    from gt4py_amd.storage.device_array import DeviceArray

    return DeviceArray(dev.view)


def bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def data(rng, domain, dtype):
    return (rng.standard_normal(domain) * 10.0 ** rng.integers(-2, 3, domain)).astype(dtype)


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def call(name: str, *args) -> None:
    lib = _lib.load()
    _lib.check(name, getattr(lib, name)(*args))


def lap5(inp: DevArray, out: DevArray, origin_in, origin_out, domain, variant=0, flags=0):
    name = "gt4mi_lap5_f64" if inp.dtype == np.float64 else "gt4mi_lap5_f32"
    call(name, _lib.domain3(domain), ctypes.byref(inp.field(origin_in)), ctypes.byref(out.field(origin_out)),
         variant, flags, stream_ptr(), None)


def hdiff(inp: DevArray, out: DevArray, coeff, origin_in, origin_out, origin_coeff, domain, flags):
    name = "gt4mi_hdiff_f64" if inp.dtype == np.float64 else "gt4mi_hdiff_f32"
    if hasattr(coeff, "field"):  # (a DevArray or anything else that describes a field: fullsize_util.StorageField)
        cf, cs = ctypes.byref(coeff.field(origin_coeff)), 0.0
    else:
        cf, cs = None, float(coeff)
    call(name, _lib.domain3(domain), ctypes.byref(inp.field(origin_in)), ctypes.byref(out.field(origin_out)),
         cf, cs, flags, stream_ptr(), None)


def tridiag(inf, diag, sup, rhs, out, origins, domain):
    name = "gt4mi_tridiag_f64" if inf.dtype == np.float64 else "gt4mi_tridiag_f32"
    fs = [ctypes.byref(a.field(origins[n])) for n, a in
          zip(("inf", "diag", "sup", "rhs", "out"), (inf, diag, sup, rhs, out))]
    call(name, _lib.domain3(domain), *fs, stream_ptr(), None)


def hdiff_ring(inp: DevArray, out: DevArray, coeff, origin_in, origin_out, origin_coeff, domain, flags, widths):
    name = "gt4mi_hdiff_ring_f64" if inp.dtype == np.float64 else "gt4mi_hdiff_ring_f32"
    if isinstance(coeff, DevArray):
        cf, cs = ctypes.byref(coeff.field(origin_coeff)), 0.0
    else:
        cf, cs = None, float(coeff)
    call(name, _lib.domain3(domain), ctypes.byref(inp.field(origin_in)), ctypes.byref(out.field(origin_out)),
         cf, cs, flags, _lib.int4(widths), stream_ptr(), None)


def lap5_ring(inp: DevArray, out: DevArray, origin_in, origin_out, domain, outer, inner, variant=0, flags=0):
    name = "gt4mi_lap5_ring_f64" if inp.dtype == np.float64 else "gt4mi_lap5_ring_f32"
    call(name, _lib.domain3(domain), ctypes.byref(inp.field(origin_in)), ctypes.byref(out.field(origin_out)),
         variant, flags, _lib.int4(outer), _lib.int4(inner), stream_ptr(), None)
