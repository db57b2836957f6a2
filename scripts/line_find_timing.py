"""What a first-crossing or extremum search along I, J or K costs (output kept as profiles/line_find_timing.txt).

Per shape, axis, number of fields and mode, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3 sets of
fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.linefind.LineFind call of all the fields (frozen form: one launch): argmax, crossing, crossing with an IJK coord;
  (a) the route a user has without it, once per field, fresh tensors each: torch.argmax plus torch.max along that dim for argmax;
      for a crossing the two compares of neighbouring items, argmax of the mask, two gathers and the arithmetic of the position
      (with a coord: two more gathers and its arithmetic).  It counts no crossings and has no rule for item 0: it does less;
  (b) gt4mi_stream_copy of as many bytes as (k) reads: (one read per field [+ the coord once]) x box x itemsize (the copy writes
      them as well; the search writes three doubles per line and field).

Bar: (k) is not slower than (a) for the same fields -- slower meaning a larger median with disjoint quartiles; the script exits
non-zero when a row misses it.  (k)/(b) is reported and carries no bar.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/line_find_timing.py, in a run of its own.
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
LEVEL = 0.25
SHAPES = (("1024x1024x80 float32", (1024, 1024, 80), np.float32),
          ("512x512x128 float64", (512, 512, 128), np.float64))
CASES = (("argmax        ", "argmax", False), ("crossing      ", "crossing", False), ("crossing+coord", "crossing", True))


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


def torch_crossing(t, z, ax, level):
    """The first crossing of `level` along dim `ax`, torch's way: (position, coord or None)."""
    import torch

    n = t.shape[ax]
    lo, hi = t.narrow(ax, 0, n - 1), t.narrow(ax, 1, n - 1)
    mask = ((lo < level) & (hi >= level)) | ((lo > level) & (hi <= level))
    q = torch.argmax(mask.to(torch.uint8), dim=ax, keepdim=True)
    a, b = torch.gather(lo, ax, q), torch.gather(hi, ax, q)
    frac = (level - a) / (b - a)
    position = q + frac
    if z is None:
        return position, None
    za, zb = torch.gather(z, ax, q), torch.gather(z, ax, q + 1)
    return position, za + frac * (zb - za)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "line_find_timing.txt"))
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, linefind

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    backend = "hip:mi300"
    lib = _lib.load()
    say(_lib.device_info())
    say(f"HIP events around single calls, {WARMUP} warm-ups, {args.calls} timed calls, {SETS} sets of fields in rotation; "
        "median [first quartile, third quartile] in microseconds")
    missed, slowest = [], (0.0, "")
    for name, shape, dtype in SHAPES:
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        itemsize = np.dtype(dtype).itemsize
        gen = torch.Generator(device="cuda").manual_seed(1)

        def storage(values):
            s = gt_storage.zeros(shape, dtype, backend=backend)
            s.tensor.copy_(values)
            return s

        def rand(lo, hi):
            return lo + (hi - lo) * torch.rand(shape, dtype=tdt, device="cuda", generator=gen)

        fields = [[storage(rand(-1, 1)) for _ in range(8)] for _ in range(SETS)]
        coords = [storage(rand(0.5, 2)) for _ in range(SETS)]
        stream = torch.cuda.current_stream().cuda_stream
        box = shape[0] * shape[1] * shape[2] * itemsize
        for ax, axis in enumerate("IJK"):
            say(f"\n{name}, lines along {axis} (n = {shape[ax]}, {shape[(ax + 1) % 3] * shape[(ax + 2) % 3]} lines)")
            for count in (1, 8):
                copies = {}
                for label, what, with_coord in CASES:
                    def baseline(s):
                        for n in range(count):
                            t = fields[s][n].tensor
                            if what == "argmax":
                                torch.argmax(t, dim=ax)
                                torch.max(t, dim=ax)
                            else:
                                torch_crossing(t, coords[s].tensor if with_coord else None, ax, LEVEL)

                    frozen = [linefind.LineFind(fields[s][:count], axis=axis, what=what, level=LEVEL if what == "crossing" else None,
                                                coord=coords[s] if with_coord else None) for s in range(SETS)]
                    assert all(f.launches == 1 for f in frozen)
                    # the same numbers?  (random items: no ties, no item on the level)
                    frozen[0]()
                    got, = frozen[0].get()[:1]
                    t = fields[0][0].tensor
                    if what == "argmax":
                        assert np.array_equal(got.position, torch.argmax(t, dim=ax).cpu().numpy().astype(np.float64)), "torch.argmax and the kernel disagree"
                        assert np.array_equal(got.value, torch.max(t, dim=ax).values.cpu().numpy().astype(np.float64)), "torch.max and the kernel disagree"
                    else:
                        position, where = torch_crossing(t, coords[0].tensor if with_coord else None, ax, LEVEL)
                        there = got.crossings > 0
                        assert there.mean() > 0.9 and np.allclose(got.position[there], position.squeeze(ax).cpu().numpy()[there], rtol=1e-5), \
                            "torch's crossing and the kernel disagree"
                        if with_coord:
                            assert np.allclose(got.coord[there], where.squeeze(ax).cpu().numpy()[there], rtol=1e-4), "torch's coord and the kernel disagree"
                        del position, where
                    del t, got
                    read = (count + (1 if with_coord else 0)) * box
                    t_a = event_us(baseline, args.calls)
                    if with_coord not in copies:
                        buf_in, buf_out = (torch.empty(read, dtype=torch.uint8, device="cuda") for _ in range(2))
                        copies[with_coord] = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), read, stream), args.calls)
                        del buf_in, buf_out
                    t_b = copies[with_coord]
                    t_k = event_us(lambda s: frozen[s](), args.calls)
                    say(f"  {count} field(s) {label}: (a) torch {show(t_a)}   (b) copy of {read / 2**20:6.0f} MiB {show(t_b)}   "
                        f"(k) LineFind ({frozen[0].path}) {show(t_k)}   {read / (t_k[1] * 1e-6) / 1e12:.2f} TB/s read; "
                        f"(k)/(a) = {t_k[1] / t_a[1]:.3f}, (k)/(b) = {t_k[1] / t_b[1]:.3f}")
                    if t_k[1] > t_a[1] and t_k[0] > t_a[2]:  # slower: the median above (a)'s, the quartiles disjoint
                        missed.append(f"{name} along {axis} {count} field(s) {label.strip()}: (k) {t_k[1]:.1f} > (a) {t_a[1]:.1f}")
                    if t_k[1] / t_b[1] > slowest[0]:
                        slowest = (t_k[1] / t_b[1], f"{name} along {axis}, {count} field(s), {label.strip()} ({frozen[0].path})")
                    del frozen
                    torch.cuda.empty_cache()
        del fields, coords
        torch.cuda.empty_cache()
    say(f"\nslowest against the copy: (k)/(b) = {slowest[0]:.3f}: {slowest[1]}")
    say(f"bar: (k) not slower than (a) by medians for the same fields -> {'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
