"""What a prefix scan along I, J or K costs (output kept as profiles/line_scan_timing.txt).

Per shape, axis, number of fields and operation, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3 sets of
fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.linescan.LineScan call of all the fields (frozen form: one launch): sum, sum with an IJK weight, max;
  (a) the route a user has without it: torch.cumsum / torch.cummax on each field's tensor (with a weight: on the product), once per
      field, a fresh result each; torch chooses the order of the additions, so its sums are not the contract's bits;
  (b) gt4mi_stream_copy of the algorithmic bytes: (1 read + 1 write per field [+ the weight once]) x box x itemsize.

Bar: (k) is not slower than (a) for the same fields -- slower meaning a larger median with disjoint quartiles; the script exits
non-zero when a row misses it.  (k)/(b) is reported and carries no bar.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/line_scan_timing.py, in a run of its own.
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
CASES = (("sum       ", "sum", False), ("sum*weight", "sum", True), ("max       ", "max", False))


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "line_scan_timing.txt"))
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, linescan

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

        def storage(values=None):
            s = gt_storage.zeros(shape, dtype, backend=backend)
            if values is not None:
                s.tensor.copy_(values)
            return s

        def rand(lo, hi):
            return lo + (hi - lo) * torch.rand(shape, dtype=tdt, device="cuda", generator=gen)

        srcs = [[storage(rand(-1, 1)) for _ in range(8)] for _ in range(SETS)]
        dsts = [[storage() for _ in range(8)] for _ in range(SETS)]
        weights = [storage(rand(0.5, 2)) for _ in range(SETS)]
        stream = torch.cuda.current_stream().cuda_stream
        box = shape[0] * shape[1] * shape[2] * itemsize
        for ax, axis in enumerate("IJK"):
            say(f"\n{name}, lines along {axis} (n = {shape[ax]}, {shape[(ax + 1) % 3] * shape[(ax + 2) % 3]} lines)")
            for count in (1, 8):
                copies = {}
                for label, op, weighted in CASES:
                    def baseline(s):
                        for n in range(count):
                            t = srcs[s][n].tensor
                            if weighted:
                                t = t * weights[s].tensor
                            if op == "sum":
                                torch.cumsum(t, ax)
                            else:
                                torch.cummax(t, ax)

                    frozen = [linescan.LineScan(dsts[s][:count], srcs[s][:count], axis=axis, op=op, weight=weights[s] if weighted else None)
                              for s in range(SETS)]
                    assert all(f.launches == 1 for f in frozen)
                    # the same numbers? max: the same bits; sum: torch's order of additions is its own
                    frozen[0]()
                    t = srcs[0][0].tensor * weights[0].tensor if weighted else srcs[0][0].tensor
                    want = torch.cumsum(t, ax) if op == "sum" else torch.cummax(t, ax).values
                    torch.cuda.synchronize()
                    if op == "max":
                        assert torch.equal(dsts[0][0].tensor, want), "torch.cummax and the kernel disagree"
                    else:
                        assert torch.allclose(dsts[0][0].tensor, want, rtol=1e-3 if dtype is np.float32 else 1e-9, atol=1e-2), \
                            "torch.cumsum and the kernel disagree"
                    del t, want
                    algorithmic = (2 * count + (1 if weighted else 0)) * box
                    t_a = event_us(baseline, args.calls)
                    if weighted not in copies:
                        half = algorithmic // 2 - (algorithmic // 2) % 16
                        buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
                        copies[weighted] = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), args.calls)
                        del buf_in, buf_out
                    t_b = copies[weighted]
                    t_k = event_us(lambda s: frozen[s](), args.calls)
                    say(f"  {count} field(s) {label}: (a) torch {show(t_a)}   (b) copy of {algorithmic / 2**20:6.0f} MiB {show(t_b)}   "
                        f"(k) LineScan ({frozen[0].path}) {show(t_k)}   {algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; "
                        f"(k)/(a) = {t_k[1] / t_a[1]:.3f}, (k)/(b) = {t_k[1] / t_b[1]:.3f}")
                    if t_k[1] > t_a[1] and t_k[0] > t_a[2]:  # slower: the median above (a)'s, the quartiles disjoint
                        missed.append(f"{name} along {axis} {count} field(s) {label.strip()}: (k) {t_k[1]:.1f} > (a) {t_a[1]:.1f}")
                    del frozen
                    torch.cuda.empty_cache()
        del srcs, dsts, weights
        torch.cuda.empty_cache()
    say(f"\nbar: (k) not slower than (a) by medians for the same fields -> {'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
