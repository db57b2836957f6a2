"""``gt4py_amd.linesolve`` -- tridiagonal solves along the lines of I, J or K, one kernel launch per 8 right-hand sides.

GTScript iterates sequentially along K only, so a recurrence along I or J -- implicit horizontal diffusion, an ADI step, a compact
finite difference, an implicit zonal filter, the line relaxation of a semi-implicit solver -- cannot be written as a stencil; the
kernel library's one Thomas solve (``tridiagonal_solver``) is K only, takes one right-hand side, rewrites its coefficients and has
no periodic closure.  ``gt4mi_line_solve`` (csrc/line_solve.hip.h) solves

    a[m] x[m-1] + b[m] x[m] + c[m] x[m+1] = d[m],   m = 0 .. n-1

for every line of the box along ``axis``, for up to eight (out, rhs) pairs per launch that share one set of coefficients, on the
current stream, without synchronisation or allocation; the elimination factors of a line are formed once for all its fields.

    from gt4py_amd import linesolve
    linesolve.solve_lines(out, rhs, lower=a, diag=b, upper=c, axis="I")
    solve = linesolve.LineSolve([u_new, v_new], [ru, rv], lower=a, diag=b, upper=c, axis="I", periodic=True)   # frozen
    for step in range(steps):
        build_rhs(u, v, ru, rv, ...)      # a stencil
        solve()                           # one call on the current stream
        physics(u_new, v_new, ...)

The coefficients are never written.  ``out[n]`` may be ``rhs[n]`` itself (an in-place solve); nothing else may overlap.  With
``periodic=True`` the line is closed (``a[0]`` couples point 0 to point n-1, ``c[n-1]`` point n-1 to point 0; n >= 3); without it
``a[0]`` and ``c[n-1]`` are never read.  The arithmetic -- the fields' dtype throughout, its order fixed, no pivoting -- is part of
the contract (include/gt4py_amd.h): the same line gives the same bits whatever the layout, the axis, the position in the call or
the device.  A rank's block must hold whole lines along ``axis``; block-tridiagonal and pentadiagonal systems and mixed dtypes are
out of scope.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from . import _lib
from ._bound import AXES, FLAGS, STREAM, Bound, Out, _coefficient, _line_pairs, field_table  # noqa: F401 - AXES is public here
from .storage.device_array import DeviceArray

PATHS = {_lib.LINE_PATH_LANES: "lanes", _lib.LINE_PATH_TILES: "tiles", _lib.LINE_PATH_ITEMS: "items"}
COEFFICIENTS = ("lower", "diag", "upper")


class LineSolve(Bound):
    """The frozen form of :func:`solve_lines` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run), the native descriptors and the workspace built once, ``__call__()`` makes only the ctypes call, on the
    stream that is current THEN.

    ``n`` is the line length, ``lines`` the number of lines, ``extent`` the IJK box (the compute domain grown by the halo in I
    and J), ``launches`` the kernels a call enqueues, ``path`` the kernel the strides select (``"lanes"``: lanes along a
    unit-stride axis other than ``axis``; ``"tiles"``: ``axis`` is the unit-stride axis, tiles go through LDS; ``"items"``:
    anything else, slow), ``workspace`` the :class:`DeviceArray` that holds the elimination factors: its layout is the library's,
    and no result depends on what it held before a call.  The object holds raw pointers and weak references to the CALLER's
    objects, not the arrays: it refuses to run once one of them has died."""

    _entry, _dry_run_bit = "gt4mi_line_solve", _lib.LINE_DRY_RUN
    _workspace_ptr, _workspace_bytes = None, 0  # (until the first dry run has said how large the workspace is)

    def _arguments(self) -> tuple:
        lower, diag, upper = self._coefficients
        return (self._out, self._rhs, self._n, ctypes.byref(lower), ctypes.byref(diag), ctypes.byref(upper), self._extent3, self._axis,
                self._size, FLAGS, self._workspace_ptr, self._workspace_bytes, STREAM, Out(ctypes.c_int64), Out(ctypes.c_int), Out(ctypes.c_int))

    def __init__(self, out, rhs, *, lower, diag, upper, axis: str = "I", periodic: bool = False, halo=0,
                 origin: Optional[Sequence[int]] = None):
        self.axis, self.periodic = axis, bool(periodic)
        #: ``extent``: the IJK box that is solved (the domain grown by the halo in I and J); ``n``, ``lines``: its lines' length and number
        (outs, rhss, o_arrays, r_arrays, c_arrays, self._halo, self.origin, self.domain, self.extent, self.n, self.lines, ax,
         start) = _line_pairs("solve_lines", out, rhs, axis, halo, origin, shared=(lower, diag, upper), names=COEFFICIENTS,
                              sharing="the fields and coefficients", roles=("out field(s)", "rhs field(s)"))
        self._n = len(o_arrays)
        self._out, self._rhs = field_table(o_arrays, start), field_table(r_arrays, start)
        self._coefficients = tuple(_coefficient(a, ax, start) for a in c_arrays)
        self._extent3 = _lib.domain3(self.extent)
        self._axis, self._size = ax, o_arrays[0].itemsize
        self._flags = _lib.LINE_PERIODIC if self.periodic else 0
        arrays = o_arrays + r_arrays + c_arrays

        def allocate(torch, device, outs):
            #: the elimination factors of every line (and, for a periodic call, the closure's solution); private layout
            self.workspace = DeviceArray(torch.empty(max(outs[0] // self._size, 1), dtype=o_arrays[0].tensor.dtype, device=device))
            self._workspace_ptr, self._workspace_bytes = self.workspace.ptr, outs[0]

        # the dry run says: the workspace the call needs, its path and how many kernels it makes
        _, path, self.launches = self._own_buffers("solve_lines", arrays, allocate)
        self.path = PATHS.get(path)
        self._bind("solve_lines", arrays, outs + rhss + [lower, diag, upper])


def solve_lines(out, rhs, *, lower, diag, upper, axis: str = "I", periodic: bool = False, halo=0,
                origin: Optional[Sequence[int]] = None) -> None:
    """Solve ``lower[m] x[m-1] + diag[m] x[m] + upper[m] x[m+1] = rhs[m]`` along every line of the compute domain (plus ``halo``
    ghost cells in I and J) along ``axis``, in one kernel launch (per 8 pairs) on the current stream.

    ``out``, ``rhs``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding.
                ``out[n]`` may be ``rhs[n]`` itself (in place); every other overlap is refused.
    ``lower``, ``diag``, ``upper``  of the fields' dtype, never written: IJK fields, or 1-d arrays of n items along ``axis``
                that every line shares (broadcast, not copied).
    ``axis``    ``"I"``, ``"J"`` or ``"K"``.
    ``periodic``  close the line: ``lower[0]`` couples point 0 to point n-1, ``upper[n-1]`` point n-1 to point 0; n >= 3.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``.
    ``origin``  first compute-domain point of every IJK array, default ``(lo_i, lo_j, 0)``.

    Allocates the workspace of the call; for a time loop build a :class:`LineSolve` once instead.  Raises ``ValueError`` /
    ``TypeError`` (with the library's message) before any GPU work."""
    LineSolve(out, rhs, lower=lower, diag=diag, upper=upper, axis=axis, periodic=periodic, halo=halo, origin=origin)()
