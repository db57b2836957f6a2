"""What a tridiagonal line solve along I or J costs (output kept as profiles/line_solve_timing.txt).

Per shape, axis and number of right-hand sides, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3 sets of
fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.linesolve.LineSolve call of all the right-hand sides (frozen form: one launch), not periodic and periodic;
  (a) the route a user has without it: transfer.FieldCopy of the coefficients and right-hand sides into arrays whose K is the line
      axis, the kernel library's `tridiagonal_solver` stencil (device_sync=False) once per right-hand side with the coefficient it
      destroys copied again each time, transfer.FieldCopy of the solutions back.  Not periodic; the periodic rows of (k) are set
      against the same route, which computes less.
  (b) gt4mi_stream_copy of the algorithmic bytes: (3 + 2 x fields) x box x itemsize.

Bar: (k) is not slower than (a) for the same fields -- slower meaning a larger median with disjoint quartiles; the script exits
non-zero when a row misses it.  (k)/(b) is reported and carries no bar.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/line_solve_timing.py, in a run of its own.
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WARMUP = 5
SETS = 3
SHAPES = (("1024x1024x80 float32", (1024, 1024, 80), np.float32),
          ("512x512x128 float64", (512, 512, 128), np.float64))
#: per axis: the shape of the array whose K is the line axis, and the permutation that views it as IJK
PERMUTED = {"I": (lambda s: (s[1], s[2], s[0]), (2, 0, 1)), "J": (lambda s: (s[0], s[2], s[1]), (0, 2, 1))}


def event_us(fn, calls):
    """(first quartile, median, third quartile) in microseconds of fn(n) over `calls` calls, n rotating over the sets of fields;
    one event pair around each call."""
    import torch

    for n in range(WARMUP):
        fn(n % SETS)
    torch.cuda.synchronize()
    pairs = []
    for c in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn(c % SETS)
        stop.record()
        pairs.append((start, stop))
    torch.cuda.synchronize()
    times = np.array([a.elapsed_time(b) for a, b in pairs]) * 1e3
    return tuple(float(v) for v in np.percentile(times, (25, 50, 75)))


def show(t):
    return f"{t[1]:10.1f}  [{t[0]:.1f}, {t[2]:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "line_solve_timing.txt"))
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, linesolve, transfer
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    backend = "hip:mi300"
    lib = _lib.load()
    say(_lib.device_info())
    say(f"HIP events around single calls, {WARMUP} warm-ups, {args.calls} timed calls, {SETS} sets of fields in rotation; "
        "median [first quartile, third quartile] in microseconds")
    missed = []
    for name, shape, dtype in SHAPES:
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        itemsize = np.dtype(dtype).itemsize
        gen = torch.Generator(device="cuda").manual_seed(1)
        tri = gtscript.stencil(backend=backend, definition=hip_templates.tridiagonal_solver, dtypes={"T": dtype}, device_sync=False)

        def storage(shp, values=None):
            s = gt_storage.zeros(shp, dtype, backend=backend)
            if values is not None:
                s.tensor.copy_(values)
            return s

        def rand(lo, hi):
            return lo + (hi - lo) * torch.rand(shape, dtype=tdt, device="cuda", generator=gen)

        # per set: diagonally dominant coefficients, 8 right-hand sides, 8 solutions
        coefs = [[storage(shape, rand(-1, 1)), storage(shape, rand(4, 5)), storage(shape, rand(-1, 1))] for _ in range(SETS)]
        rhss = [[storage(shape, rand(-1, 1)) for _ in range(8)] for _ in range(SETS)]
        outs = [[storage(shape) for _ in range(8)] for _ in range(SETS)]
        stream = torch.cuda.current_stream().cuda_stream
        for axis in ("I", "J"):
            to_shape, perm = PERMUTED[axis]
            pshape = to_shape(shape)
            # the arrays of route (a): K is the line axis; `view` shows one of them as the IJK array it is a permuted copy of
            p_coefs = [[storage(pshape) for _ in range(3)] for _ in range(SETS)]
            p_sup = [storage(pshape) for _ in range(SETS)]
            p_rhss = [[storage(pshape) for _ in range(8)] for _ in range(SETS)]
            p_outs = [[storage(pshape) for _ in range(8)] for _ in range(SETS)]
            # (the views are kept: a frozen call holds weak references to what it was given)
            v_coefs = [[p.tensor.permute(*perm) for p in p_coefs[s]] for s in range(SETS)]
            v_rhss = [[p.tensor.permute(*perm) for p in p_rhss[s]] for s in range(SETS)]
            v_outs = [[p.tensor.permute(*perm) for p in p_outs[s]] for s in range(SETS)]
            say(f"\n{name}, lines along {axis} (n = {shape['IJK'.index(axis)]})")
            for count in (1, 8):
                there = [transfer.FieldCopy(v_coefs[s] + v_rhss[s][:count], coefs[s] + rhss[s][:count]) for s in range(SETS)]
                again = [transfer.FieldCopy(p_sup[s], p_coefs[s][2]) for s in range(SETS)]
                back = [transfer.FieldCopy(outs[s][:count], v_outs[s][:count]) for s in range(SETS)]

                def baseline(s):
                    there[s]()
                    for n in range(count):
                        again[s]()  # (the stencil rewrites sup and rhs in place)
                        tri(p_coefs[s][0], p_coefs[s][1], p_sup[s], p_rhss[s][n], p_outs[s][n])
                    back[s]()

                frozen = {periodic: [linesolve.LineSolve(outs[s][:count], rhss[s][:count], lower=coefs[s][0], diag=coefs[s][1], upper=coefs[s][2],
                                                         axis=axis, periodic=periodic) for s in range(SETS)] for periodic in (False, True)}
                assert all(f.launches == 1 for fs in frozen.values() for f in fs)
                # the same numbers? (the same arithmetic: the same bits)
                baseline(0)
                check = outs[0][0].tensor.clone()
                frozen[False][0]()
                torch.cuda.synchronize()
                assert torch.equal(outs[0][0].tensor, check), "the baseline and the kernel disagree"
                algorithmic = (3 + 2 * count) * shape[0] * shape[1] * shape[2] * itemsize
                t_a = event_us(baseline, args.calls)
                say(f"  {count} rhs: (a) copies + tridiagonal_solver per rhs + copy back   {show(t_a)}")
                half = algorithmic // 2 - (algorithmic // 2) % 16
                buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
                t_b = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), args.calls)
                say(f"  {count} rhs: (b) gt4mi_stream_copy, {algorithmic / 2**20:6.0f} MiB in + out          {show(t_b)}")
                del buf_in, buf_out
                for periodic in (False, True):
                    fs = frozen[periodic]
                    t_k = event_us(lambda s: fs[s](), args.calls)
                    say(f"  {count} rhs: (k) LineSolve {'periodic' if periodic else 'open    '} ({fs[0].path}), one launch      {show(t_k)}   "
                        f"{algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; (k)/(a) = {t_k[1] / t_a[1]:.3f}, (k)/(b) = {t_k[1] / t_b[1]:.3f}")
                    if t_k[1] > t_a[1] and t_k[0] > t_a[2]:  # slower: the median above (a)'s, the quartiles disjoint
                        missed.append(f"{name} along {axis} {count} rhs {'periodic' if periodic else 'open'}: (k) {t_k[1]:.1f} > (a) {t_a[1]:.1f}")
                del there, again, back, frozen
            del p_coefs, p_sup, p_rhss, p_outs, v_coefs, v_rhss, v_outs
            torch.cuda.empty_cache()
        del coefs, rhss, outs
        torch.cuda.empty_cache()
    say(f"\nbar: (k) not slower than (a) by medians for the same fields -> {'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
