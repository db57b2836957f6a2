"""What a boundary-condition halo fill costs in front of a stencil (output kept as profiles/halo_fill_timing.txt).

Per configuration and mode, side by side (HIP events, 5 warm-ups, 60 timed calls, rotating over enough fields that the
Infinity Cache does not serve repeats -- BASELINE.md section 4):
  1. the single launch of gt4py_amd.boundary.HaloFill (frozen form);
  2. the same result through DeviceArray.__setitem__ slice assignments, I sides first, then J sides (periodic: one
     assignment per side, 4 launches; zero gradient: one per ghost plane, 4 x width);
  3. gt4mi_stream_copy of as many bytes as the fill writes, for scale;
  4. the stencil the fill precedes on the same fields, and the fill's share of it.

Every timed window is ONE call of ~10 us under its own event pair: these are call-to-call figures that include the launch.
Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/halo_fill_timing.py (profiles/halo_fill_rocprofv3_kernel_stats.csv).

    python scripts/halo_fill_timing.py [--calls 60]
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

WARMUP = 5


def event_ms(fn, calls, nfields):
    """Mean time of fn(n) over `calls` calls, n rotating over the fields; one event pair around each call."""
    import torch

    for n in range(WARMUP):
        fn(n % nfields)
    torch.cuda.synchronize()
    pairs = []
    for c in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn(c % nfields)
        stop.record()
        pairs.append((start, stop))
    torch.cuda.synchronize()
    times = sorted(a.elapsed_time(b) for a, b in pairs)
    return float(np.mean(times)), times[len(times) // 2]


def slice_fill(d, w, n, modes):
    """The parent's route: slice assignments through DeviceArray.__setitem__ (periodic / zero_gradient), I first, then J."""
    ni, nj = n
    for axis, mode in enumerate(modes):
        size = (ni, nj)[axis]

        def sl(lo, hi):
            return (slice(lo, hi), slice(w, w + nj)) if axis == 0 else (slice(None), slice(lo, hi))

        if mode == "periodic":
            d[sl(0, w)] = d[sl(size, size + w)]
            d[sl(w + size, 2 * w + size)] = d[sl(w, 2 * w)]
        else:  # zero_gradient: one assignment per ghost plane
            for g in range(w):
                d[sl(g, g + 1)] = d[sl(w, w + 1)]
                d[sl(w + size + g, w + size + g + 1)] = d[sl(w + size - 1, w + size)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, boundary
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend = "hip:mi300"
    lib = _lib.load()
    print(_lib.device_info())
    print(f"HIP events, {WARMUP} warm-ups, {args.calls} timed calls; mean (median) in microseconds")
    worst_ratio = 0.0
    for name, domain, dtype, w in (("hdiff 1024x1024x80 float32, width 2", (1024, 1024, 80), np.float32, 2),
                                   ("lap5 512x512x128 float64, width 1", (512, 512, 128), np.float64, 1)):
        shape = (domain[0] + 2 * w, domain[1] + 2 * w, domain[2])
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        nfields = max(4, int(np.ceil(1.5 * 2**30 / nbytes)))  # > 1 GiB in rotation: 4x the 256 MiB Infinity Cache
        fields = [gt_storage.zeros(shape, dtype, backend=backend, aligned_index=(w, w, 0)) for _ in range(nfields)]
        gen = torch.Generator(device="cuda").manual_seed(1)
        for f in fields:
            f.tensor.copy_(torch.rand(shape, dtype=f.tensor.dtype, device="cuda", generator=gen))
        out = gt_storage.zeros(shape, dtype, backend=backend, aligned_index=(w, w, 0))
        if w == 2:
            coeff = gt_storage.full(shape, 0.1, dtype, backend=backend, aligned_index=(w, w, 0))
            st = gtscript.stencil(backend=backend, definition=hip_templates.hdiff_limiter_field, dtypes={"T": dtype}, device_sync=False)
            stencil = lambda n: st(fields[n], out, coeff, origin=(w, w, 0))  # noqa: E731
        else:
            st = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": dtype}, device_sync=False)
            stencil = lambda n: st(fields[n], out, origin=(w, w, 0), domain=domain)  # noqa: E731
        t_stencil = event_ms(stencil, args.calls, nfields)
        ghost = (shape[0] * shape[1] - domain[0] * domain[1]) * domain[2] * np.dtype(dtype).itemsize
        copy_bytes = -(-ghost // 16) * 16
        src = torch.empty(copy_bytes * nfields, dtype=torch.uint8, device="cuda")
        dst = torch.empty(copy_bytes, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        t_copy = event_ms(lambda n: lib.gt4mi_stream_copy(src.data_ptr() + n * copy_bytes, dst.data_ptr(), copy_bytes, stream),
                          args.calls, nfields)
        print(f"\n{name}: {nfields} fields of {nbytes / 2**20:.0f} MiB in rotation, {ghost / 2**20:.2f} MiB of ghost cells per field")
        print(f"  (4) the stencil alone                       {t_stencil[0] * 1e3:9.1f} ({t_stencil[1] * 1e3:.1f})")
        print(f"  (3) gt4mi_stream_copy of the ghost bytes    {t_copy[0] * 1e3:9.1f} ({t_copy[1] * 1e3:.1f})")
        for modes in (("periodic", "periodic"), ("zero_gradient", "zero_gradient")):
            frozen = [boundary.HaloFill([f], halo=w, mode=modes) for f in fields]
            assert all(f.launches == 1 for f in frozen)
            t_one = event_ms(lambda n: frozen[n](), args.calls, nfields)
            t_slices = event_ms(lambda n: slice_fill(fields[n], w, domain[:2], modes), args.calls, nfields)
            # same result? (on a field of its own, from the same start)
            a, b = fields[0], fields[1]
            b.tensor.copy_(a.tensor)
            frozen[0]()
            slice_fill(b, w, domain[:2], modes)
            assert torch.equal(a.tensor, b.tensor), "the slice assignments and the single launch disagree"
            ratio = t_one[0] / t_slices[0]
            worst_ratio = max(worst_ratio, ratio)
            print(f"  {modes[0]}:")
            print(f"  (1) HaloFill, one launch                    {t_one[0] * 1e3:9.1f} ({t_one[1] * 1e3:.1f})   "
                  f"= {100 * t_one[0] / t_stencil[0]:.1f} % of (4)")
            print(f"  (2) slice assignments (DeviceArray.__setitem__) {t_slices[0] * 1e3:5.1f} ({t_slices[1] * 1e3:.1f})   "
                  f"= {100 * t_slices[0] / t_stencil[0]:.1f} % of (4);  (1) / (2) = {ratio:.3f}")
        del fields, frozen, src, dst
        torch.cuda.empty_cache()
    print(f"\nacceptance: (1) no slower than (2) in every row: worst (1) / (2) = {worst_ratio:.3f} -> "
          f"{'met' if worst_ratio <= 1.0 else 'NOT met'}")
    return 0 if worst_ratio <= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
