"""What the per-level statistics of a field cost (output kept as profiles/level_stats_timing.txt).

Per shape, side by side (HIP events around single calls, 5 warm-ups, 40 timed calls, 8 fields in rotation so that the 256 MiB
Infinity Cache does not serve repeats; median and quartiles):
  (a) one gt4py_amd.diagnostics.LevelStats call of one field (frozen form: the pass and the finishing launch);
  (b) the route a user has without it, kept on the device: widen to float64, then per level sum, abs().sum, (x*x).sum, amin,
      amax and the isfinite count over dim=(0, 1) -- the same profiles, nothing copied to the host;
  (c) one diagnostics.FieldStats call of the same field in the same process (the whole-field form);
  (d) gt4mi_stream_copy of the field's byte span: the same bytes in AND out.

Bar: (a) <= (b) by medians on every shape, no margin beyond the quartiles printed; the script exits non-zero when it is
missed.  (a)/(c) and (a)/(d) are reported and carry no bar.

The tiles-per-level constant LT (GT4MI_LEVEL_STATS_MAX_TILES) is fixed at build time.  To compare values, build the library
with another one into a directory of its own and point GT4PY_AMD_LIB at it; --routes a --append adds that run's (a) rows:

    make -C gt4py_amd/csrc LIBDIR=$PWD/gt4py_amd/lib/lt64 DEFS=-DGT4MI_LEVEL_STATS_MAX_TILES=64
    python scripts/level_stats_timing.py
    GT4PY_AMD_LIB=gt4py_amd/lib/lt64/libgt4py_amd.so python scripts/level_stats_timing.py --routes a --append

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/level_stats_timing.py, in a run of its own.
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WARMUP = 5
NFIELDS = 8
HBM_PEAK = 8.0e12  # bytes per second
SHAPES = (("512x512x512 float64, halo 1", (512, 512, 512), np.float64, 1),
          ("512x512x128 float64, halo 1", (512, 512, 128), np.float64, 1),
          ("1024x1024x80 float32, halo 2", (1024, 1024, 80), np.float32, 2))


def event_us(fn, calls):
    """(first quartile, median, third quartile) in microseconds of fn(n) over `calls` calls, n rotating over the fields; one
    event pair around each call."""
    import torch

    for n in range(WARMUP):
        fn(n % NFIELDS)
    torch.cuda.synchronize()
    pairs = []
    for c in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn(c % NFIELDS)
        stop.record()
        pairs.append((start, stop))
    torch.cuda.synchronize()
    times = np.array([a.elapsed_time(b) for a, b in pairs]) * 1e3
    return tuple(float(v) for v in np.percentile(times, (25, 50, 75)))


def torch_route(view):
    """The same profiles from torch reductions, results left on the device."""
    import torch

    x = view.double()
    return (x.sum(dim=(0, 1)), x.abs().sum(dim=(0, 1)), (x * x).sum(dim=(0, 1)), x.amin(dim=(0, 1)), x.amax(dim=(0, 1)),
            torch.isfinite(x).sum(dim=(0, 1)))


def show(t):
    return f"{t[1]:10.1f}  [{t[0]:.1f}, {t[2]:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--routes", default="abcd", help="which of the routes a, b, c, d to time")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "level_stats_timing.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, diagnostics

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    backend = "hip:mi300"
    lib = _lib.load()
    say(_lib.device_info())
    say(f"HIP events around single calls, {WARMUP} warm-ups, {args.calls} timed calls, {NFIELDS} fields in rotation; "
        "median [first quartile, third quartile] in microseconds")
    missed = []
    for name, domain, dtype, w in SHAPES:
        shape = (domain[0] + 2 * w, domain[1] + 2 * w, domain[2])
        itemsize = np.dtype(dtype).itemsize
        nbytes = int(np.prod(shape)) * itemsize
        domain_bytes = int(np.prod(domain)) * itemsize
        fields = [gt_storage.zeros(shape, dtype, backend=backend, aligned_index=(w, w, 0)) for _ in range(NFIELDS)]
        gen = torch.Generator(device="cuda").manual_seed(1)
        for f in fields:
            f.tensor.copy_(torch.rand(shape, dtype=f.tensor.dtype, device="cuda", generator=gen))
        views = [f.tensor[w:-w, w:-w] for f in fields]
        frozen = [diagnostics.LevelStats([f], halo=w) for f in fields]
        assert all(f.launches == 2 for f in frozen)
        tiles = frozen[0]._workspace_bytes // (domain[2] * 64)
        rows_per_wave = -(-domain[1] // (4 * tiles))
        # the same numbers? counts and extremes exactly, sums within the rounding of two different orders
        frozen[0]()
        p, = frozen[0].get()
        ref = [v.cpu().numpy() for v in torch_route(views[0])]
        plane = domain[0] * domain[1]
        assert (p.count == plane).all() and np.array_equal(p.nonfinite, plane - ref[5])
        assert np.array_equal(p.min, ref[3]) and np.array_equal(p.max, ref[4])
        assert np.allclose(p.sum, ref[0], rtol=1e-9) and np.allclose(p.sum_sq, ref[2], rtol=1e-9) and np.allclose(p.mean, ref[0] / plane, rtol=1e-9)
        say(f"\n{name}: {NFIELDS} fields of {nbytes / 2**20:.0f} MiB in rotation, {domain_bytes / 2**20:.0f} MiB of domain per field; "
            f"{tiles} tiles per level = {tiles * domain[2]} workgroups, {rows_per_wave} rows per wave")
        t = {}
        if "a" in args.routes:
            t["a"] = event_us(lambda n: frozen[n](), args.calls)
            rate = domain_bytes / (t["a"][1] * 1e-6)
            say(f"  (a) LevelStats, one field (2 launches), {tiles:3d} tiles per level {show(t['a'])}   "
                f"reads {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak")
        if "b" in args.routes:
            t["b"] = event_us(lambda n: torch_route(views[n]), args.calls)
            say(f"  (b) six torch reductions over dim=(0, 1), on the device     {show(t['b'])}")
        if "c" in args.routes:
            whole = [diagnostics.FieldStats([f], halo=w) for f in fields]
            t["c"] = event_us(lambda n: whole[n](), args.calls)
            say(f"  (c) FieldStats, one field (2 launches)                      {show(t['c'])}")
        if "d" in args.routes:
            stride = fields[0].strides
            span = (domain[0] - 1) * stride[0] + (domain[1] - 1) * stride[1] + (domain[2] - 1) * stride[2] + itemsize
            span -= span % 16
            dst = torch.empty(span, dtype=torch.uint8, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            starts = [f.ptr + (-f.ptr) % 16 for f in fields]
            t["d"] = event_us(lambda n: lib.gt4mi_stream_copy(starts[n], dst.data_ptr(), span, stream), args.calls)
            say(f"  (d) gt4mi_stream_copy of the byte span                      {show(t['d'])}   "
                f"({2 * span / (t['d'][1] * 1e-6) / 1e12:.2f} TB/s in + out)")
            del dst
        if "a" in t:
            ratios = [f"(a) / ({r}) = {t['a'][1] / t[r][1]:.3f}" for r in "bcd" if r in t]
            if ratios:
                say("      medians: " + ", ".join(ratios))
            if "b" in t and t["a"][1] > t["b"][1]:
                missed.append(f"{name}: (a) {t['a'][1]:.1f} > (b) {t['b'][1]:.1f}")
        del fields, views, frozen
        torch.cuda.empty_cache()
    if "a" in args.routes and "b" in args.routes:
        say(f"\nbar: (a) <= (b) by medians on every shape -> {'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a" if args.append else "w") as fh:
        fh.write("\n".join(lines) + "\n" + ("\n" if args.append else ""))
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
