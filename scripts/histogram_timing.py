"""What a histogram of fields costs (output kept as profiles/histogram_timing.txt).

Per shape, number of fields, number of bins, kind of edges, whole box or per level, and kind of data, side by side (HIP events
around single calls, 5 warm-ups, 30 timed calls, 3 sets of fields in rotation so that the 256 MiB Infinity Cache does not serve
repeats; median and quartiles):
  (k) one gt4py_amd.histogram.Histogram call of all the fields (frozen form: a memset and one launch);
  (a) the route a user has without it, once per field, fresh tensors each: torch.histc where the edges are uniform and the box
      is one row, else torch.bucketize + torch.bincount (per level the level's offset is added before the bincount).  It keeps
      no below / above / nan counters apart and closes no last bin: it does less;
  (b) one diagnostics.FieldStats call on the same fields: the project's read-only pass over the same bytes.

Bar: every row of (k) beats (a) -- a smaller median; the script exits non-zero when a row misses it.  (k)/(b) is reported and
carries no bar.

Every shape runs in a child process of its own under a time limit; a child that fails or runs out of time ends the run.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/histogram_timing.py --shape 0, in a run of its own.
"""

from __future__ import annotations

import argparse
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WARMUP = 5
SETS = 3
LIMIT = 420  # seconds a shape may take
SHAPES = (("1024x1024x80 float32", (1024, 1024, 80), np.float32),
          ("512x512x128 float64", (512, 512, 128), np.float64))
HI = 50.0  # the range of the data: [0, HI], "mm per hour"


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
    return f"{t[1]:9.1f} [{t[0]:.1f}, {t[2]:.1f}]"


def edges_of(kind, nb):
    return np.linspace(0.0, HI, nb + 1) if kind == "uniform" else np.concatenate([[0.0], np.logspace(-3, np.log10(HI), nb)])


def one_shape(index, calls, say):
    """The rows of one shape.  Returns the rows that miss the bar."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics, histogram

    name, shape, dtype = SHAPES[index]
    if index == 0:
        from gt4py_amd import _lib

        say(_lib.device_info())
    tdt = torch.float32 if dtype is np.float32 else torch.float64
    gen = torch.Generator(device="cuda").manual_seed(1)
    ni, nj, nk = shape
    i, j, k = (torch.arange(n, dtype=tdt, device="cuda") for n in shape)

    def storage(values):
        s = gt_storage.zeros(shape, dtype, backend="hip:mi300")
        s.tensor.copy_(values)
        return s

    def smooth(n):  # neighbouring items share a bin more often than not; every bin of the range is met
        wave = torch.sin(i * (0.002 + 0.0003 * n))[:, None, None] * torch.cos(j * 0.0031)[None, :, None]
        return (0.5 * HI * (0.8 * wave + 1.0) + 0.1 * HI * (k / nk)[None, None, :] - 0.05 * HI).clamp_(0.0, HI)

    def mostly_zero(n):
        u = torch.rand(shape, dtype=tdt, device="cuda", generator=gen)
        return torch.where(u < 0.9, torch.zeros((), dtype=tdt, device="cuda"), HI * torch.rand(shape, dtype=tdt, device="cuda", generator=gen))

    missed = []
    for data, make in (("smooth", smooth), ("90 % zeros", mostly_zero)):
        fields = [[storage(make(8 * s + n)) for n in range(8)] for s in range(SETS)]
        for count in (1, 8):
            stats = [diagnostics.FieldStats(fields[s][:count]) for s in range(SETS)]
            t_b = event_us(lambda s: stats[s](), calls)
            say(f"\n{name}, {data}, {count} field(s): (b) FieldStats {show(t_b)}")
            del stats
            for nb in (64, 1024):
                for kind in ("uniform", "log"):
                    e = edges_of(kind, nb)
                    bounds = torch.from_numpy(e[1:-1].copy()).to(device="cuda", dtype=tdt)  # nb - 1 inner edges: indices 0 .. nb - 1
                    offsets = (torch.arange(nk, device="cuda") * nb)[None, None, :]
                    for by in (None, "K"):
                        def baseline(s):
                            for n in range(count):
                                t = fields[s][n].tensor
                                if by is None and kind == "uniform":
                                    torch.histc(t, bins=nb, min=0.0, max=HI)
                                elif by is None:
                                    torch.bincount(torch.bucketize(t, bounds, right=True).reshape(-1), minlength=nb)
                                else:
                                    torch.bincount((torch.bucketize(t, bounds, right=True) + offsets).reshape(-1), minlength=nb * nk)

                        frozen = [histogram.Histogram(fields[s][:count], edges=e, by=by) for s in range(SETS)]
                        # the same numbers?  (all items are inside the edges; an item ON an edge may differ between the routes, so
                        # the bucketize route, which compares against the same float64 edges rounded to the type, is the one compared)
                        frozen[0]()
                        got = frozen[0].get()[0]
                        assert np.all(got.total == (ni * nj if by else ni * nj * nk)) and np.sum(got.inside) == ni * nj * nk, "items are missing"
                        if dtype is np.float64:
                            t = fields[0][0].tensor
                            ref = torch.bincount((torch.bucketize(t, bounds, right=True) + (offsets if by else 0)).reshape(-1),
                                                 minlength=nb * (nk if by else 1)).cpu().numpy().reshape(got.counts.shape)
                            assert np.array_equal(got.counts, ref), "torch's route and the kernel disagree"
                            del t, ref
                        t_a = event_us(baseline, calls)
                        t_k = event_us(lambda s: frozen[s](), calls)
                        verdict = "" if t_k[1] < t_a[1] else "   MISSES the bar"
                        say(f"  nb {nb:4d} {kind:7s} {'per level' if by else 'whole box'}: (a) torch {show(t_a)}   (k) Histogram ({frozen[0].path}) "
                            f"{show(t_k)}   (k)/(a) = {t_k[1] / t_a[1]:.3f}, (k)/(b) = {t_k[1] / t_b[1]:.2f}{verdict}")
                        if verdict:
                            missed.append(f"{name} {data} {count} field(s) nb {nb} {kind} {'per level' if by else 'whole box'}: "
                                          f"(k) {t_k[1]:.1f} >= (a) {t_a[1]:.1f}")
                        del frozen
                        torch.cuda.empty_cache()
        del fields
        torch.cuda.empty_cache()
    return missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "histogram_timing.txt"))
    ap.add_argument("--shape", type=int, default=None, help="run the rows of one shape in this process and print them")
    args = ap.parse_args()
    if args.shape is not None:
        missed = one_shape(args.shape, args.calls, lambda text="": print(text, flush=True))
        for m in missed:
            print(f"MISSED: {m}", flush=True)
        return 0
    # (this process starts the children and never opens the device itself)
    lines = [f"HIP events around single calls, {WARMUP} warm-ups, {args.calls} timed calls, {SETS} sets of fields in rotation; "
             "median [first quartile, third quartile] in microseconds"]
    print("\n".join(lines), flush=True)
    missed = []
    for index in range(len(SHAPES)):
        try:
            child = subprocess.run([sys.executable, __file__, "--shape", str(index), "--calls", str(args.calls)], timeout=LIMIT,
                                   stdout=subprocess.PIPE, text=True)  # (warnings go to the terminal, not to the file)
        except subprocess.TimeoutExpired as exc:
            print(exc.stdout or "", flush=True)
            print(f"shape {index} ran out of its {LIMIT} s: nothing more is started", flush=True)
            return 2
        print(child.stdout, flush=True)
        if child.returncode != 0:
            print(f"shape {index} ended with status {child.returncode}: nothing more is started", flush=True)
            return 2
        for text in child.stdout.splitlines():
            if text.startswith("MISSED: "):
                missed.append(text[len("MISSED: "):])
            else:
                lines.append(text)
    lines.append(f"\nbar: every row of (k) beats (a) by medians for the same fields -> {'met' if not missed else 'MISSES: ' + '; '.join(missed)}")
    print(lines[-1], flush=True)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
