"""What the frozen utility calls (``boundary.HaloFill``, ``diagnostics.FieldStats`` / ``LevelStats``, ``transfer.FieldCopy``,
``vertical.VerticalRemap`` / ``VerticalInterp``, ``horizontal.HorizontalInterp`` / ``HorizontalRemap``, ``departure.DepartureInterp``, ``sampling.Sample``, ``linesolve.LineSolve``, ``linescan.LineScan``, ``linefind.LineFind``, ``linefilter.LineFilter`` / ``LineSpectrum``, ``histogram.Histogram``) share on the Python side: turning a refusal of the library into an
exception, normalising halo / origin / domain / field lists, the native field tables, the dry run, and binding a checked call to
the caller's objects.

A new utility is a subclass of :class:`Bound` that states ``_entry`` (the C entry's name), ``_dry_run_bit`` (the entry's
``*_DRY_RUN`` flag) and ``_arguments()``: the entry's argument list, written ONCE, with :data:`FLAGS` and :data:`STREAM` where the
flags and the stream go and an :class:`Out` where the entry takes an out-pointer (``launches``, ``workspace_needed``, ``path``,
``paths``).  Its constructor checks what only Python can say (names, dtypes, dimensions, the messages in its own words), builds
the descriptors (:func:`field_table`, :func:`_common_domain`), sets ``_flags`` where the object has flags of its own, calls
:meth:`Bound._dry_run` -- every check of the library on exactly that list, nothing enqueued, the out values returned -- and
:meth:`Bound._bind` last.  ``__call__`` is the base's: the same list with the object's flags, the stream that is current then and
null out-pointers.

A utility WITH RESULTS is a subclass of :class:`BoundResult`, whose ``__call__`` keeps the stream; its ``get()`` opens with
:meth:`BoundResult._wait` (the refusal before the first call, then the synchronisation) and reads ``result``.  Buffers that the
object owns and that the entry takes as pointers beside its fields (a result, a workspace, a table) are null class attributes
that ``_arguments()`` reads; where the constructor would call ``_dry_run``, it calls :meth:`Bound._own_buffers` with a function
that allocates them and sets the pointers -- the library's refusals come first, the host-array refusal second, an allocation last.
A device view of one entry checks its index with :meth:`Bound._index`, and the synchronous function is :func:`one_shot`."""

from __future__ import annotations

import ctypes
import weakref
from typing import NoReturn, Sequence, Tuple

import numpy as np

from . import _lib
from .storage.device_array import DeviceArray, as_device_array

FLOATS = (np.dtype("float32"), np.dtype("float64"))


def raise_refusal(func: str, rc: int) -> NoReturn:
    """A non-zero status of entry ``func`` as an exception with the library's message: ``ValueError``, ``TypeError`` for what
    no kernel handles (``ERR_UNSUPPORTED``), :class:`~gt4py_amd._lib.NativeError` for a HIP error."""
    message = _lib.load().gt4mi_last_error().decode("utf-8", "replace")
    if rc == _lib.ERR_HIP:
        raise _lib.NativeError(func, rc, message)
    raise (TypeError if rc == _lib.ERR_UNSUPPORTED else ValueError)(message)


def _halo4(halo) -> Tuple[int, int, int, int]:
    def integer(x):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise TypeError(f"halo widths must be ints, not {type(x).__name__}")
        return int(x)

    if isinstance(halo, (int, np.integer)):
        h = integer(halo)
        return h, h, h, h
    if not isinstance(halo, (tuple, list)) or len(halo) != 2:
        raise ValueError(f"halo must be an int, (hi, hj) or ((lo_i, hi_i), (lo_j, hi_j)), not {halo!r}")
    out = []
    for axis in halo:
        if isinstance(axis, (tuple, list)):
            if len(axis) != 2:
                raise ValueError(f"halo must be an int, (hi, hj) or ((lo_i, hi_i), (lo_j, hi_j)), not {halo!r}")
            out += [integer(axis[0]), integer(axis[1])]
        else:
            out += [integer(axis)] * 2
    return tuple(out)  # type: ignore[return-value]


def _as_list(fields) -> list:
    """One field or a sequence of fields (a tuple or list; an array is ONE field whatever its length)."""
    return list(fields) if isinstance(fields, (tuple, list)) else [fields]


def _triple(value, name: str, fill: int) -> Tuple[int, int, int]:
    value = tuple(int(v) for v in value)
    if len(value) > 3:
        raise ValueError(f"{name} must have at most three entries, not {value}")
    return value + (fill,) * (3 - len(value))  # type: ignore[return-value]


def _shape3(a: DeviceArray) -> Tuple[int, ...]:
    return tuple(a.shape) + (1,) * (3 - a.ndim)


def _origin3(origin, halo4) -> Tuple[int, int, int]:
    """``origin`` as three ints; by default the first point behind the low ghost cells."""
    return (halo4[0], halo4[2], 0) if origin is None else _triple(origin, "origin", 0)


def _box_of(first: DeviceArray, halo4, origin, domain, least: int):
    """(origin, domain) of a call whose fields share both: ``domain`` defaults to what ``first`` has left behind ``origin`` and in
    front of its high ghost cells, which must be at least ``least`` points along every axis."""
    origin = _origin3(origin, halo4)
    if domain is None:
        domain = tuple(s - o - h for s, o, h in zip(_shape3(first), origin, (halo4[1], halo4[3], 0)))
        if min(domain) < least:
            raise ValueError(f"halo {halo4} and origin {origin} leave no domain in a field of shape {first.shape}")
    return origin, _triple(domain, "domain", 1)


def _common_domain(arrays, halo4, origin, listed, axes: int = 3, least_k: int = 0) -> Tuple[int, ...]:
    """The common compute domain along the first ``axes`` axes: what every one of ``arrays`` has left behind ``origin`` and (in I and
    J) in front of its high ghost cells, over the axes it has.  ``listed``: the arrays whose shapes the refusal names; ``least_k``:
    the fewest levels (where ``axes`` is 3)."""
    high = (halo4[1], halo4[3], 0)
    domain = tuple(min(a.shape[x] - origin[x] - high[x] for a in arrays if a.ndim > x) for x in range(axes))
    if min(domain) < 0 or (axes == 3 and domain[2] < least_k):
        raise ValueError(f"halo {halo4} and origin {origin} leave no domain in fields of shapes {[a.shape for a in listed]}")
    return domain


def field_table(arrays, start):
    """The native ``_lib.Field`` table of ``arrays`` (IJK, or IJ: one level), every box starting at ``start``."""
    table = (_lib.Field * len(arrays))()
    for n, a in enumerate(arrays):
        table[n] = _lib.Field.make(a.ptr, _shape3(a), tuple(a.strides) + (0,) * (3 - a.ndim), start)
    return table


def _pair_lists(who: str, dst, src, halo, method=None, methods=None, shared=(), roles=("destination(s)", "source(s)")):
    """The opening of a call on (dst, src) pairs, in the order the checks have always had: two lists of equal length, a known
    ``method`` (where there are ``methods``), DeviceArrays of everything (``shared``: fields every pair reads), the halo.
    ``roles``: what the length message calls the two lists.
    Returns (dsts, srcs, dst arrays, src arrays, shared arrays, halo4)."""
    dsts, srcs = _as_list(dst), _as_list(src)
    if not dsts or not srcs:
        raise ValueError(f"{who} needs at least one pair of fields")
    if len(dsts) != len(srcs):
        raise ValueError(f"{who} pairs fields one to one: {len(dsts)} {roles[0]} and {len(srcs)} {roles[1]} were passed")
    if methods is not None and method not in methods:
        raise ValueError(f"method must be one of {sorted(methods)}, not {method!r}")
    d_arrays = [as_device_array(f) for f in dsts]
    s_arrays = [as_device_array(f) for f in srcs]
    x_arrays = [as_device_array(f) for f in shared]
    halo4 = _halo4(halo)
    if min(halo4) < 0:
        raise ValueError(f"halo widths must not be negative: {halo4}")
    return dsts, srcs, d_arrays, s_arrays, x_arrays, halo4


def _float_pairs(who: str, dst, src, halo, method, methods, *, shared, names: Sequence[str], ndims, kind: str, plural: str):
    """:func:`_pair_lists` for IJK fields of ONE float dtype and the shared fields ``names`` (of ``ndims`` dimensions: IJK or a
    ``kind``; one tuple for all of them or one tuple per field, ``(3,)`` for a field that must be IJK) of one float dtype of their
    own; ``plural`` is what the last message calls them."""
    dsts, srcs, d_arrays, s_arrays, x_arrays, halo4 = _pair_lists(who, dst, src, halo, method, methods, shared)
    for a in d_arrays + s_arrays:
        if a.ndim != 3:
            raise ValueError(f"{who} takes IJK fields, not a field of {a.ndim} dimension(s)")
    per_field = ndims if isinstance(ndims[0], tuple) else (ndims,) * len(names)
    for name, a, allowed in zip(names, x_arrays, per_field):
        if a.ndim not in allowed:
            raise ValueError(f"{name} must be an IJK field{f' or a {kind}' if len(allowed) > 1 else ''}, not a field of {a.ndim} dimension(s)")
    dtype = d_arrays[0].dtype
    for a in d_arrays + s_arrays:
        if a.dtype != dtype:
            raise TypeError(f"the fields of one call share a dtype: {dtype} and {a.dtype} differ")
    if dtype not in FLOATS:
        raise TypeError(f"{who} takes float32 or float64 fields, not {dtype}")
    for name, a in zip(names[1:], x_arrays[1:]):
        if a.dtype != x_arrays[0].dtype:
            raise TypeError(f"{names[0]} and {name} share a dtype: {x_arrays[0].dtype} and {a.dtype} differ")
    if x_arrays[0].dtype not in FLOATS:
        raise TypeError(f"{plural} are float32 or float64, not {x_arrays[0].dtype}")
    return dsts, srcs, d_arrays, s_arrays, x_arrays, halo4


#: the line axes of ``solve_lines``, ``scan_lines`` and (with 0, 1, 2 and lower case as well) ``line_stats`` and ``find_lines``
AXES = {"I": 0, "J": 1, "K": 2}


def _axis_index(axis) -> int:
    """``"I"``, ``"J"``, ``"K"`` or 0, 1, 2 as 0, 1, 2."""
    if isinstance(axis, str) and axis.upper() in AXES:
        return AXES[axis.upper()]
    if not isinstance(axis, bool) and isinstance(axis, (int, np.integer)) and 0 <= int(axis) <= 2:
        return int(axis)
    raise ValueError(f"axis must be 'I', 'J', 'K' or 0, 1, 2, not {axis!r}")


def _coefficient(a: DeviceArray, axis: int, start) -> "_lib.Field":
    """A field every line reads: IJK, or 1-d along ``axis`` (broadcast: stride 0 along the two other axes)."""
    if a.ndim == 1:  # n items along the line axis: every line reads the same ones
        shape, strides, origin = [1, 1, 1], [0, 0, 0], [0, 0, 0]
        shape[axis], strides[axis] = a.shape[0], a.strides[0]
        return _lib.Field.make(a.ptr, shape, strides, origin)
    return _lib.Field.make(a.ptr, a.shape, a.strides, start)


def _line_pairs(who: str, dst, src, axis, halo, origin, *, shared, names: Sequence[str], sharing: str, own_checks=None,
                roles=("destination(s)", "source(s)")):
    """:func:`_pair_lists` for a call along the lines of ``axis``, in the order the checks have always had: the axis,
    ``own_checks()`` (the caller's other names), IJK fields and shared fields ``names`` that are IJK or 1-d along the axis, ONE
    float dtype (``sharing``: what its message calls them), the common compute domain -- along the line axis the arrays must
    agree, a line is never cut short silently -- and the length of every 1-d shared field.  Adds to what :func:`_pair_lists`
    returns: origin, domain, ``extent`` (the IJK box: the domain grown by the halo in I and J), ``n`` (the line length),
    ``lines`` (how many the box holds), ``ax`` (the axis as 0, 1, 2), ``start`` (the box's first point in every IJK array)."""
    dsts, srcs, d_arrays, s_arrays, x_arrays, halo4 = _pair_lists(who, dst, src, halo, shared=shared, roles=roles)
    if axis not in AXES:
        raise ValueError(f"axis must be one of {sorted(AXES)}, not {axis!r}")
    if own_checks is not None:
        own_checks()
    ax = AXES[axis]
    for a in d_arrays + s_arrays:
        if a.ndim != 3:
            raise ValueError(f"{who} takes IJK fields, not a field of {a.ndim} dimension(s)")
    for name, a in zip(names, x_arrays):
        if a.ndim not in (1, 3):
            raise ValueError(f"{name} must be an IJK field or a 1-d array along {axis}, not a field of {a.ndim} dimension(s)")
    dtype = d_arrays[0].dtype
    for a in d_arrays + s_arrays + x_arrays:
        if a.dtype != dtype:
            raise TypeError(f"{sharing} of one call share a dtype: {dtype} and {a.dtype} differ")
    if dtype not in FLOATS:
        raise TypeError(f"{who} takes float32 or float64 fields, not {dtype}")
    lo_i, hi_i, lo_j, hi_j = halo4
    origin = _origin3(origin, halo4)
    full = [a for a in d_arrays + s_arrays + x_arrays if a.ndim == 3]
    domain = _common_domain(full, halo4, origin, full, least_k=1)
    for a in full:
        have = a.shape[ax] - origin[ax] - (hi_i, hi_j, 0)[ax]
        if have != domain[ax]:
            raise ValueError(f"the fields of one call share their length along {axis}: {domain[ax]} and {have} differ")
    extent = (domain[0] + lo_i + hi_i, domain[1] + lo_j + hi_j, domain[2])
    n, lines = extent[ax], extent[(ax + 1) % 3] * extent[(ax + 2) % 3]
    for name, a in zip(names, x_arrays):
        if a.ndim == 1 and a.shape[0] != n:
            raise ValueError(f"{name} has {a.shape[0]} items, a line of {n} points along {axis} needs {n}")
    start = (origin[0] - lo_i, origin[1] - lo_j, origin[2])
    return dsts, srcs, d_arrays, s_arrays, x_arrays, halo4, origin, domain, extent, n, lines, ax, start


def refuse_host_arrays(who: str, arrays) -> None:
    for a in arrays:
        if not a.tensor.is_cuda:
            raise TypeError(f"{who} works on device fields; a host array was passed")


#: the slots of an argument list that the dry run and the call fill differently
FLAGS, STREAM = object(), object()


class Out:
    """An out-pointer slot of an argument list: a ``ctype`` the entry writes one of, or an array type it fills."""

    def __init__(self, ctype):
        self.ctype = ctype


def dry_run(entry: str, dry_run_bit: int, flags: int, arguments) -> list:
    """Entry ``entry`` on ``arguments`` with ``dry_run_bit`` set in the flags, a null stream and real out-pointers: every check of
    the library, nothing enqueued.  A refusal becomes ``ValueError`` (``TypeError`` for what no kernel handles) with the library's
    message.  Returns what the entry left behind the out-pointers, in their order (an array as a list)."""
    outs = []

    def slot(a):
        if a is FLAGS:
            return flags | dry_run_bit
        if a is STREAM:
            return None
        if isinstance(a, Out):
            outs.append(a.ctype())
            return outs[-1] if isinstance(outs[-1], ctypes.Array) else ctypes.byref(outs[-1])
        return a

    rc = getattr(_lib.load(), entry)(*[slot(a) for a in arguments])
    if rc != _lib.OK:
        raise_refusal(entry, rc)
    return [list(o) if isinstance(o, ctypes.Array) else o.value for o in outs]


class Bound:
    """Base of the frozen calls: a constructor builds the native descriptors, checks them through the library's dry run
    (:meth:`_dry_run`) and calls :meth:`_bind` last; ``__call__`` is :meth:`_check_alive` and the one ctypes call, both on the
    argument list that :meth:`_arguments` states."""

    _entry = ""        # the C entry
    _dry_run_bit = 0   # its *_DRY_RUN flag
    _flags = 0         # the flags of the object's own calls

    def _arguments(self) -> tuple:
        """The entry's arguments in order, :data:`FLAGS`, :data:`STREAM` and :class:`Out` where those go."""
        raise NotImplementedError

    def _dry_run(self) -> list:
        return dry_run(self._entry, self._dry_run_bit, self._flags, self._arguments())

    def _own_buffers(self, who: str, arrays, allocate) -> list:
        """The dry run of a call with buffers of its own, whose pointers are still null: every check of the library, nothing
        enqueued; then ``allocate(torch, device, outs)`` -- the device of the first of ``arrays``, what the dry run returned --
        makes the buffers and sets the pointers.  Returns what that dry run returned.  ``who``, ``arrays``: as for :meth:`_bind`."""
        outs = self._dry_run()
        refuse_host_arrays(who, arrays)  # (nothing is allocated for a call that cannot be bound)
        import torch

        allocate(torch, arrays[0].tensor.device, outs)
        self._dry_run()  # the buffers against the fields (overlap, alignment): the dry run once more, now with them
        return outs

    def _index(self, entry, noun: str = "entry") -> int:
        """``entry`` as an index into the ``_n`` entries of the call; ``noun``: what the refusal calls them."""
        entry = int(entry)
        if not 0 <= entry < self._n:
            raise IndexError(f"{noun} {entry} of {self._n}")
        return entry

    def _bind(self, who: str, arrays, objects) -> None:
        """``who``: the public function's name; ``arrays``: the DeviceArrays of the call; ``objects``: what the caller passed."""
        refuse_host_arrays(who, arrays)  # (last: none of the checks before needs a device)
        # the call's arguments, built once: all but the stream, which is the one current at the call
        arguments = [self._flags if a is FLAGS else None if isinstance(a, Out) else a for a in self._arguments()]
        at = next(n for n, a in enumerate(arguments) if a is STREAM)
        self._before, self._after = tuple(arguments[:at]), tuple(arguments[at + 1:])
        # what must stay alive is what the CALLER holds: for a torch tensor or another exporter `as_device_array` made a wrapper
        # that dies with the constructor, so the weak reference goes to the object that was passed; one that cannot be weakly
        # referenced is held instead
        self._refs, self._held = [], []
        for f in objects:
            try:
                self._refs.append(weakref.ref(f))
            except TypeError:
                self._held.append(f)
        import torch

        self._current_stream = torch.cuda.current_stream
        self._native = getattr(_lib.load(), self._entry)

    def __call__(self) -> None:
        self._check_alive()
        rc = self._native(*self._before, self._current_stream().cuda_stream, *self._after)
        if rc != _lib.OK:
            _lib.check(self._entry, rc)

    def _check_alive(self) -> None:
        for r in self._refs:  # (a plain loop: this runs in front of every call)
            if r() is None:
                name = type(self).__name__
                raise RuntimeError(f"{name}: an array this call was bound to no longer exists; build a new {name}")


class BoundResult(Bound):
    """A frozen call whose ``get()`` brings a result to the host: the call keeps its stream for it."""

    _stream = None  # the stream of the last direct call

    def __call__(self) -> None:  # (Bound's, in one frame of its own: this is the host time of a call)
        self._check_alive()
        self._stream = self._current_stream()  # (kept for get())
        rc = self._native(*self._before, self._stream.cuda_stream, *self._after)
        if rc != _lib.OK:
            _lib.check(self._entry, rc)

    def _wait(self) -> None:
        """What ``get()`` opens with: ``RuntimeError`` before the first call, else it waits for the stream of the last DIRECT call
        (``self._stream``) and the stream that is current now.  A replay of a captured graph is no call of the object: it runs on
        the stream it is replayed on, while ``self._stream`` still names the capture's stream, on which nothing ran.  So: call
        ``get()`` with the replay's stream current (or synchronise that stream first)."""
        if self._stream is None:
            raise RuntimeError(f"{type(self).__name__}.get: the object has not been called yet")
        self._stream.synchronize()
        current = self._current_stream()
        if current != self._stream:
            current.synchronize()


def one_shot(frozen_class, fields, **kwargs):
    """The synchronous form of a frozen call with results: ``fields`` are the positional arguments as the public function got
    them, the fields themselves or one list or tuple of them; freeze, call, get."""
    fields = list(fields[0]) if len(fields) == 1 and isinstance(fields[0], (tuple, list)) else list(fields)
    frozen = frozen_class(fields, **kwargs)
    frozen()
    return frozen.get()
