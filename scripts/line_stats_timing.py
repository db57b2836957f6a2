"""What statistics along the lines of I, J or K cost (output kept as profiles/line_stats_timing.txt).

Per shape and axis, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 8 fields in rotation so that the
256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (a1) one gt4py_amd.diagnostics.LineStats call of one field (frozen form: the pass and, for lines of several segments, the
       finishing launch);  (a8) one call of eight fields;
  (b1) the route a user has without it, kept on the device: widen to float64, then sum, abs().sum, (x*x).sum, amin, amax and the
       isfinite count over that dim -- the same sections, nothing copied to the host;  (b8) the same for eight fields;
  (c)  one diagnostics.LevelStats call of the same field in the same process;
  (d)  gt4mi_stream_copy of the field's byte span: the same bytes in AND out.

Bar: (a1) < (b1) and (a8) < (b8) by medians on every row; the script exits non-zero when a row misses it and names the row.
(a1)/(c) and (a1)/(d) are reported and carry no bar.  The ratio is against torch, never against this code.

The segment length G (GT4MI_LINE_STATS_SEGMENT) is fixed at build time.  To compare values, build the library with another one
into a directory of its own and point GT4PY_AMD_LIB at it; --routes a --append adds that run's (a) rows:

    make -C gt4py_amd/csrc LIBDIR=$PWD/gt4py_amd/lib/g64 DEFS=-DGT4MI_LINE_STATS_SEGMENT=64
    python scripts/line_stats_timing.py
    GT4PY_AMD_LIB=gt4py_amd/lib/g64/libgt4py_amd.so python scripts/line_stats_timing.py --routes a --append

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/line_stats_timing.py, in a run of its own.
"""

from __future__ import annotations

import argparse
import ctypes
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WARMUP = 5
NFIELDS = 8
HBM_PEAK = 8.0e12  # bytes per second
SHAPES = (("1024x1024x80 float32, halo 2", (1024, 1024, 80), np.float32, 2),
          ("512x512x512 float64, halo 1", (512, 512, 512), np.float64, 1))


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


def torch_route(view, dim):
    """The same sections from torch reductions, results left on the device."""
    import torch

    x = view.double()
    return (x.sum(dim=dim), x.abs().sum(dim=dim), (x * x).sum(dim=dim), x.amin(dim=dim), x.amax(dim=dim), torch.isfinite(x).sum(dim=dim))


def segment_items(lib, _lib):
    """G of the library that is loaded: the longest line of one segment (asked of the dry run)."""
    for g in (2 ** e for e in range(2, 16)):
        f = _lib.Field.make(0x10000, (g + 1, 1, 1), (8, 8 * (g + 1), 8 * (g + 1)), (0, 0, 0))
        needed = ctypes.c_int64()
        rc = lib.gt4mi_line_stats(ctypes.byref(f), None, 1, _lib.domain3((g + 1, 1, 1)), 0, 8, None, 0, None, _lib.STATS_DRY_RUN, None,
                                  ctypes.byref(needed), None, None)
        assert rc == 0
        if needed.value == 2 * 64:
            return g
    raise RuntimeError("no segment length found")


def show(t):
    return f"{t[1]:10.1f}  [{t[0]:.1f}, {t[2]:.1f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--routes", default="abcd", help="which of the routes a, b, c, d to time")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "line_stats_timing.txt"))
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
    g = segment_items(lib, _lib)
    say(_lib.device_info())
    say(f"G = GT4MI_LINE_STATS_SEGMENT = {g}.  HIP events around single calls, {WARMUP} warm-ups, {args.calls} timed calls, {NFIELDS} fields "
        "in rotation; median [first quartile, third quartile] in microseconds")
    missed = []
    paths = {_lib.LINE_STATS_PATH_LANES: "LANES", _lib.LINE_STATS_PATH_TILES: "TILES", _lib.LINE_STATS_PATH_ITEMS: "ITEMS"}
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
        say(f"\n{name}: {NFIELDS} fields of {nbytes / 2**20:.0f} MiB in rotation, {domain_bytes / 2**20:.0f} MiB of domain per field")
        for axis in range(3):
            n = domain[axis]
            frozen = [diagnostics.LineStats([f], axis=axis, halo=w) for f in fields]
            eight = diagnostics.LineStats(fields, axis=axis, halo=w)
            # the same numbers? counts and extremes exactly, sums within the rounding of two different orders
            frozen[0]()
            p, = frozen[0].get()
            ref = [v.cpu().numpy() for v in torch_route(views[0], axis)]
            assert (p.count == n).all() and np.array_equal(p.nonfinite, n - ref[5])
            assert np.array_equal(p.min, ref[3]) and np.array_equal(p.max, ref[4])
            assert np.allclose(p.sum, ref[0], rtol=1e-9) and np.allclose(p.sum_sq, ref[2], rtol=1e-9) and np.allclose(p.mean, ref[0] / n, rtol=1e-9)
            say(f"  along {'IJK'[axis]} (n = {n}, {-(-n // g)} segments, path {paths[frozen[0].path]}, {frozen[0].launches} launches):")
            t = {}
            if "a" in args.routes:
                t["a1"] = event_us(lambda k: frozen[k](), args.calls)
                rate = domain_bytes / (t["a1"][1] * 1e-6)
                say(f"    (a1) LineStats, one field             {show(t['a1'])}   reads {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak")
                t["a8"] = event_us(lambda k: eight(), args.calls)
                rate = NFIELDS * domain_bytes / (t["a8"][1] * 1e-6)
                say(f"    (a8) LineStats, eight fields, one call {show(t['a8'])}   reads {rate / 1e12:.2f} TB/s")
            if "b" in args.routes:
                t["b1"] = event_us(lambda k: torch_route(views[k], axis), args.calls)
                say(f"    (b1) six torch reductions over dim={axis}  {show(t['b1'])}")
                t["b8"] = event_us(lambda k: [torch_route(v, axis) for v in views], args.calls)
                say(f"    (b8) the same for eight fields         {show(t['b8'])}")
            if "c" in args.routes:
                level = [diagnostics.LevelStats([f], halo=w) for f in fields]
                t["c"] = event_us(lambda k: level[k](), args.calls)
                say(f"    (c)  LevelStats, one field             {show(t['c'])}")
                del level
            if "d" in args.routes:
                stride = fields[0].strides
                span = (domain[0] - 1) * stride[0] + (domain[1] - 1) * stride[1] + (domain[2] - 1) * stride[2] + itemsize
                span -= span % 16
                dst = torch.empty(span, dtype=torch.uint8, device="cuda")
                stream = torch.cuda.current_stream().cuda_stream
                starts = [f.ptr + (-f.ptr) % 16 for f in fields]
                t["d"] = event_us(lambda k: lib.gt4mi_stream_copy(starts[k], dst.data_ptr(), span, stream), args.calls)
                say(f"    (d)  gt4mi_stream_copy of the byte span {show(t['d'])}   ({2 * span / (t['d'][1] * 1e-6) / 1e12:.2f} TB/s in + out)")
                del dst
            if "a1" in t:
                ratios = [f"({x}) / ({y}) = {t[x][1] / t[y][1]:.3f}" for x, y in (("a1", "b1"), ("a8", "b8"), ("a1", "c"), ("a1", "d")) if y in t]
                if ratios:
                    say("         medians: " + ", ".join(ratios))
                for x, y in (("a1", "b1"), ("a8", "b8")):
                    if y in t and not t[x][1] < t[y][1]:
                        missed.append(f"{name} along {'IJK'[axis]}: ({x}) {t[x][1]:.1f} >= ({y}) {t[y][1]:.1f}")
            del frozen, eight
        del fields, views
        torch.cuda.empty_cache()
    if "a" in args.routes and "b" in args.routes:
        say(f"\nbar: (a1) < (b1) and (a8) < (b8) by medians on every row -> {'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a" if args.append else "w") as fh:
        fh.write("\n".join(lines) + "\n" + ("\n" if args.append else ""))
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
