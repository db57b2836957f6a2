"""``gt4py_amd.transfer`` -- moving fields between layouts and between device and host, one kernel launch per 8 fields.

The reference moves data in and out of its storages with numpy / cupy slicing and ``cp.asarray`` on storages that ARE numpy /
cupy arrays.  The storages of this backend are :class:`~gt4py_amd.storage.DeviceArray`\\ s in an I-contiguous, row-padded layout;
a generic strided copy between that layout and a buffer in numpy's C order (K fastest) is a full 3-d transpose by a kernel that
knows neither layout.  ``gt4mi_field_copy`` (csrc/field_copy.hip.h) copies the box of up to eight (dst, src) pairs of ANY
layouts in one launch on the current stream -- through on-chip tiles where the two sides are contiguous along different axes --
without synchronisation or allocation.

    from gt4py_amd import transfer
    transfer.copy_fields(dst, src, halo=2)                    # one call: compute domain + 2 ghost cells in I and J
    cp = transfer.FieldCopy([a, b], [c, d])                   # frozen: descriptors built once
    out = transfer.Download([u, v], halo=0, dtype=np.float32) # output every n steps, read back a step late
    for step in range(steps):
        ...
        if step % n == 0:
            if pending is not None:
                write(pending.get())                          # waits for ITS copy only; C-contiguous views of pinned memory
            pending = out()                                   # enqueues layout conversion + device-to-host copy, does not wait
    up = transfer.Upload([u], halo=2)
    up([host_u])                                              # pinned staging + host-to-device copy + one launch into the box

Bit patterns are moved (bool and integer fields work, NaN payloads and the sign of zero survive); with ``convert`` / ``dtype``
float64 -> float32 is one rounding to nearest even and float32 -> float64 is exact.
"""

from __future__ import annotations

import ctypes
from typing import Any, List, Optional, Sequence

import numpy as np

from . import _lib
from ._bound import (FLAGS, FLOATS as _FLOATS, STREAM, Bound, Out, _as_list, _halo4, _origin3, _pair_lists, _shape3, _triple, dry_run, field_table,
                     refuse_host_arrays)
from .storage.device_array import DeviceArray, as_device_array, torch_dtype

PATH_ROWS, PATH_TILES, PATH_ITEMS = _lib.COPY_PATH_ROWS, _lib.COPY_PATH_TILES, _lib.COPY_PATH_ITEMS
PATH_NAMES = {PATH_ROWS: "rows", PATH_TILES: "tiles", PATH_ITEMS: "items"}


def _copy_arguments(dst, src, n: int, extent, dsize: int, ssize: int) -> tuple:
    """The argument list of ``gt4mi_field_copy``: of a :class:`FieldCopy`, and of the dry run a staged transfer makes before it has
    anything to copy to."""
    return dst, src, n, extent, dsize, ssize, FLAGS, STREAM, Out(ctypes.c_int * n), Out(ctypes.c_int)


def _conversion(dst_dtype: np.dtype, src_dtype: np.dtype, convert: bool, who: str) -> int:
    """The flags of a call from the two dtypes; anything but equal dtypes or (with ``convert``) float32 <-> float64 is refused."""
    if dst_dtype == src_dtype:
        return 0
    if not convert:
        raise TypeError(f"{who}: dtypes {src_dtype} (src) and {dst_dtype} (dst) differ; pass convert=True for float32 <-> float64")
    if dst_dtype not in _FLOATS or src_dtype not in _FLOATS:
        raise TypeError(f"{who}: only float32 <-> float64 can be converted, not {src_dtype} to {dst_dtype}")
    return _lib.COPY_CONVERT


class FieldCopy(Bound):
    """The frozen form of :func:`copy_fields` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run) and the native descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is
    current THEN.

    ``paths`` tells which path of the kernel every pair takes (``PATH_ROWS`` / ``PATH_TILES`` / ``PATH_ITEMS``), ``launches`` how
    many kernels a call enqueues.  The object holds raw pointers and weak references to the CALLER's objects, not the arrays:
    it refuses to run once one of them has died.  (An exporter that cannot be weakly referenced is held instead.)"""

    _entry, _dry_run_bit = "gt4mi_field_copy", _lib.COPY_DRY_RUN

    def _arguments(self) -> tuple:
        return _copy_arguments(self._dst, self._src, self._n, self._extent3, self._dsize, self._ssize)

    def __init__(self, dsts, srcs, *, halo=0, origin: Optional[Sequence[int]] = None, domain: Optional[Sequence[int]] = None,
                 convert: bool = False, dst_origin: Optional[Sequence[int]] = None, src_origin: Optional[Sequence[int]] = None):
        dsts, srcs, d_arrays, s_arrays, _, self._halo = _pair_lists("copy_fields", dsts, srcs, halo)
        for a in d_arrays + s_arrays:
            if a.ndim not in (2, 3):
                raise ValueError(f"copy_fields takes IJ or IJK fields, not a field of {a.ndim} dimension(s)")
        for side, arrays in (("destinations", d_arrays), ("sources", s_arrays)):
            for a in arrays:
                if a.dtype != arrays[0].dtype:
                    raise TypeError(f"the {side} of one call share a dtype: {arrays[0].dtype} and {a.dtype} differ")
        self._flags = _conversion(d_arrays[0].dtype, s_arrays[0].dtype, bool(convert), "copy_fields")
        self._dsize, self._ssize = d_arrays[0].itemsize, s_arrays[0].itemsize
        lo_i, hi_i, lo_j, hi_j = self._halo
        default = _origin3(origin, self._halo)
        d_origin = default if dst_origin is None else _triple(dst_origin, "dst_origin", 0)
        s_origin = default if src_origin is None else _triple(src_origin, "src_origin", 0)
        if domain is None:
            # the common compute domain: what every array has left behind its origin and in front of its high ghost cells
            rest = [tuple(s - o - h for s, o, h in zip(_shape3(a), org, (hi_i, hi_j, 0)))
                    for arrays, org in ((d_arrays, d_origin), (s_arrays, s_origin)) for a in arrays]
            domain = tuple(min(r[ax] for r in rest) for ax in range(3))
            if min(domain) < 0:
                raise ValueError(f"halo {self._halo} and origins {d_origin} (dst) / {s_origin} (src) leave no domain in fields of "
                                 f"shapes {[a.shape for a in d_arrays + s_arrays]}")
        domain = _triple(domain, "domain", 1)
        self.domain, self.dst_origin, self.src_origin = domain, d_origin, s_origin
        #: the box that is copied: the domain grown by the halo in I and J
        self.extent = (domain[0] + lo_i + hi_i, domain[1] + lo_j + hi_j, domain[2])
        self._n = len(d_arrays)
        self._dst, self._src = (field_table(arrays, (org[0] - lo_i, org[1] - lo_j, org[2])) for arrays, org in ((d_arrays, d_origin), (s_arrays, s_origin)))
        self._extent3 = _lib.domain3(self.extent)
        # every check of the library, nothing enqueued; also: which paths, how many kernels
        self.paths, self.launches = self._dry_run()
        self._bind("copy_fields", d_arrays + s_arrays, dsts + srcs)


def copy_fields(dst, src, *, halo=0, origin: Optional[Sequence[int]] = None, domain: Optional[Sequence[int]] = None,
                convert: bool = False, dst_origin: Optional[Sequence[int]] = None, src_origin: Optional[Sequence[int]] = None) -> None:
    """Copy the compute domain (plus ``halo`` ghost cells in I and J) of ``src`` to ``dst``, whatever the two layouts, in one
    kernel launch (per 8 pairs) on the current stream.

    ``dst``, ``src``  one field each or two sequences of equal length: :class:`DeviceArray`\\ s (IJK, or IJ) or anything
                ``as_device_array`` accepts; every field may differ in address, strides and padding.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``.
    ``origin``  first compute-domain point on both sides, default ``(lo_i, lo_j, 0)``; ``dst_origin`` / ``src_origin`` set one
                side's own.  ``domain`` defaults to the largest that fits every field.
    ``convert`` allow float64 -> float32 (rounded to nearest even) and float32 -> float64 (exact).

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`FieldCopy` once instead."""
    FieldCopy(dst, src, halo=halo, origin=origin, domain=domain, convert=convert, dst_origin=dst_origin, src_origin=src_origin)()


class _Staged:
    """What :class:`Download` and :class:`Upload` share: per slot a device staging buffer that is dense in numpy's C order and a
    pinned host buffer of the same bytes, the frozen copy between the fields' boxes and the staging buffer, and an event."""

    def __init__(self, fields, halo, host_dtype, slots: int, origin, domain, download: bool):
        who = type(self).__name__
        fields = _as_list(fields)
        if not fields:
            raise ValueError(f"{who} needs at least one field")
        if isinstance(slots, bool) or not isinstance(slots, (int, np.integer)) or slots < 1:
            raise ValueError(f"slots must be a positive int, not {slots!r}")
        arrays = [as_device_array(f) for f in fields]
        for a in arrays:
            if a.ndim not in (2, 3):
                raise ValueError(f"{who} takes IJ or IJK fields, not a field of {a.ndim} dimension(s)")
            if a.dtype != arrays[0].dtype:
                raise TypeError(f"the fields of one {who} share a dtype: {arrays[0].dtype} and {a.dtype} differ")
        self.field_dtype = arrays[0].dtype
        self.dtype = self.field_dtype if host_dtype is None else np.dtype(host_dtype)
        pair = (self.dtype, self.field_dtype) if download else (self.field_dtype, self.dtype)
        _conversion(pair[0], pair[1], True, who)
        halo4 = _halo4(halo)
        if min(halo4) < 0:
            raise ValueError(f"halo widths must not be negative: {halo4}")
        lo_i, hi_i, lo_j, hi_j = halo4
        origin = _origin3(origin, halo4)
        if domain is None:
            rest = [tuple(s - o - h for s, o, h in zip(_shape3(a), origin, (hi_i, hi_j, 0))) for a in arrays]
            domain = tuple(min(r[ax] for r in rest) for ax in range(3))
            if min(domain) < 0:
                raise ValueError(f"halo {halo4} and origin {origin} leave no domain in fields of shapes {[a.shape for a in arrays]}")
        domain = _triple(domain, "domain", 1)
        self.origin, self.domain = origin, domain
        box = (domain[0] + lo_i + hi_i, domain[1] + lo_j + hi_j, domain[2])
        if min(box) < 1:
            raise ValueError(f"{who}: empty box {box}")
        # the library's own checks of the fields' side (bounds, strides) before anything is allocated: a dry run against made-up
        # staging addresses in C order, far from the fields
        self._check_fields(arrays, halo4, origin, domain, box, download)
        refuse_host_arrays(who, arrays)
        import torch

        self._torch = torch
        self.box = box
        #: what ``get()`` returns / ``__call__`` takes per field: the box, without a K axis for an IJ field
        self.shapes = [box if a.ndim == 3 else box[:2] for a in arrays]
        self._n, self.slots = len(arrays), int(slots)
        device = arrays[0].tensor.device
        tdt = torch_dtype(self.dtype)
        self._device_stage = [torch.empty((self._n,) + box, dtype=tdt, device=device) for _ in range(self.slots)]
        self._host_stage = [torch.empty((self._n,) + box, dtype=tdt, pin_memory=True) for _ in range(self.slots)]
        self._host_numpy = [h.numpy() for h in self._host_stage]
        self._events = [torch.cuda.Event() for _ in range(self.slots)]
        self._busy = [False] * self.slots      # an event was recorded for the slot and nobody has waited for it yet
        self._ticket = [0] * self.slots        # how many turns the slot has had: a handle of an earlier turn is stale
        self._stage_views = [[stage[n] for n in range(self._n)] for stage in self._device_stage]  # (kept alive: FieldCopy holds weak references)
        kwargs = dict(halo=halo, domain=domain, convert=True)
        stage_origin = (lo_i, lo_j, 0)
        if download:
            self._copies = [FieldCopy(views, fields, src_origin=origin, dst_origin=stage_origin, **kwargs) for views in self._stage_views]
        else:
            self._copies = [FieldCopy(fields, views, dst_origin=origin, src_origin=stage_origin, **kwargs) for views in self._stage_views]
        self.paths, self.launches = self._copies[0].paths, self._copies[0].launches
        self._turn = 0

    def _check_fields(self, arrays, halo4, origin, domain, box, download: bool) -> None:
        n = len(arrays)
        lo_i, _, lo_j, _ = halo4
        stage = (_lib.Field * n)()
        size = self.dtype.itemsize
        strides = (box[1] * box[2] * size, box[2] * size, size)
        nbytes = box[0] * strides[0]
        top = max(a.ptr + sum(abs(s) * (m - 1) for s, m in zip(a.strides, a.shape)) + a.itemsize for a in arrays)
        base = -(-top // 4096) * 4096 + 4096  # (made-up addresses behind the last field: never dereferenced in a dry run)
        fields = field_table(arrays, (origin[0] - lo_i, origin[1] - lo_j, origin[2]))
        for k in range(n):
            stage[k] = _lib.Field.make(base + k * (-(-nbytes // 4096) * 4096), box, strides, (0, 0, 0))
        sides = (stage, fields, n, _lib.domain3(box), size, self.field_dtype.itemsize) if download else \
                (fields, stage, n, _lib.domain3(box), self.field_dtype.itemsize, size)
        dry_run(FieldCopy._entry, FieldCopy._dry_run_bit, _lib.COPY_CONVERT if self.dtype != self.field_dtype else 0, _copy_arguments(*sides))

    def _next_slot(self) -> int:
        """The slot whose turn it is, free to be overwritten: whatever was enqueued on it before has completed."""
        slot = self._turn % self.slots
        self._turn += 1
        if self._busy[slot]:
            self._events[slot].synchronize()
            self._busy[slot] = False
        self._ticket[slot] += 1
        return slot

    def _host_views(self, slot: int) -> List[np.ndarray]:
        return [self._host_numpy[slot][n].reshape(shape) for n, shape in enumerate(self.shapes)]


class Transfer:
    """What :class:`Download` returns: ``get()`` waits for THIS transfer only and returns one C-contiguous numpy array per field,
    views of the slot's pinned buffer -- valid until the slot's next turn (``slots`` calls later)."""

    __slots__ = ("_owner", "_slot", "_ticket")

    def __init__(self, owner: _Staged, slot: int):
        self._owner, self._slot, self._ticket = owner, slot, owner._ticket[slot]

    def _check(self) -> None:
        if self._owner._ticket[self._slot] != self._ticket:
            raise RuntimeError(f"this transfer's slot has been reused: with slots={self._owner.slots} a handle must be read before "
                               f"the {self._owner.slots}. call after its own")

    def done(self) -> bool:
        """Whether ``get()`` would return without waiting."""
        self._check()
        return not self._owner._busy[self._slot] or bool(self._owner._events[self._slot].query())

    def get(self) -> List[np.ndarray]:
        self._check()
        owner = self._owner
        if owner._busy[self._slot]:
            owner._events[self._slot].synchronize()
            owner._busy[self._slot] = False
        return owner._host_views(self._slot)


class Download(_Staged):
    """Device-to-host transfer of the boxes (compute domain + ``halo`` ghost cells in I and J) of ``fields``, built once.

    ``__call__()`` enqueues, on the current stream, ONE ``gt4mi_field_copy`` from the fields (whatever their layout) to a device
    staging buffer that is dense in numpy's C order, then one non-blocking copy to pinned host memory and an event; it does not
    wait and returns a :class:`Transfer`.  ``dtype=np.float32`` narrows float64 fields on the way (output files).  With
    ``slots`` buffers that many transfers can be in flight; a call whose slot still holds an unread transfer waits for that
    transfer's event first, and the unread handle then refuses to be read."""

    def __init__(self, fields, *, halo=0, dtype=None, slots: int = 2, origin: Optional[Sequence[int]] = None,
                 domain: Optional[Sequence[int]] = None):
        super().__init__(fields, halo, dtype, slots, origin, domain, download=True)

    def __call__(self) -> Transfer:
        slot = self._next_slot()
        self._copies[slot]()
        self._host_stage[slot].copy_(self._device_stage[slot], non_blocking=True)
        self._events[slot].record(self._torch.cuda.current_stream())
        self._busy[slot] = True
        return Transfer(self, slot)


class Upload(_Staged):
    """Host-to-device transfer into the boxes (compute domain + ``halo`` ghost cells in I and J) of ``fields``, built once.

    ``__call__(host_arrays)`` checks shapes and dtypes, copies the arrays into the slot's pinned buffer, enqueues the
    host-to-device copy to the staging buffer and ONE ``gt4mi_field_copy`` into the fields' boxes, on the current stream, and
    does not wait.  Ghost cells outside the box, row padding and slack are not written.  ``dtype=np.float32`` takes float32
    host arrays for float64 fields (widened exactly)."""

    def __init__(self, fields, *, halo=0, dtype=None, slots: int = 2, origin: Optional[Sequence[int]] = None,
                 domain: Optional[Sequence[int]] = None):
        super().__init__(fields, halo, dtype, slots, origin, domain, download=False)

    def __call__(self, host_arrays) -> None:
        host_arrays = _as_list(host_arrays)
        if len(host_arrays) != self._n:
            raise ValueError(f"Upload was built for {self._n} field(s), {len(host_arrays)} host array(s) were passed")
        for n, (h, shape) in enumerate(zip(host_arrays, self.shapes)):
            if not isinstance(h, np.ndarray):
                raise TypeError(f"Upload takes numpy arrays, not {type(h).__name__} (array {n})")
            if h.dtype != self.dtype:
                raise TypeError(f"host array {n} has dtype {h.dtype}, this Upload takes {self.dtype}")
            if tuple(h.shape) != tuple(shape):
                raise ValueError(f"host array {n} has shape {h.shape}, the box is {tuple(shape)}")
        slot = self._next_slot()
        for view, h in zip(self._host_views(slot), host_arrays):
            np.copyto(view, h)
        self._device_stage[slot].copy_(self._host_stage[slot], non_blocking=True)
        self._copies[slot]()
        self._events[slot].record(self._torch.cuda.current_stream())
        self._busy[slot] = True
