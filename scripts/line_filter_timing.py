"""What a Fourier filter along I or J costs (output kept as profiles/line_filter_timing.txt).

Per shape, axis, number of fields and form of the response, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3
sets of fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.linefilter.LineFilter call of all the fields (frozen form: one launch), with a response that every line shares and
      with one per index of another axis (along I: per latitude, (nj, 1, nh); along J: per level, (1, nk, nh));
  (a) the route a user has without it: torch.fft.rfft, a multiply and torch.fft.irfft on each field's tensor (the same DeviceArray
      views), once per field, fresh complex intermediates each; the FFT library chooses the arithmetic and works in the fields' own
      precision, so its results are not the contract's bits;
  (b) gt4mi_stream_copy of the algorithmic bytes: (1 read + 1 write per field) x box x itemsize.

Bar: (k) takes less time than (a) per field, by medians.  Every row is written down with `met` or `MISSED`; (k)/(b) is reported and
carries no bar.  The script exits 0 either way: the rows are the record.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/line_filter_timing.py, in a run of its own.
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "line_filter_timing.txt"))
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, linefilter

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    backend = "hip:mi300"
    lib = _lib.load()
    say(_lib.device_info())
    say(f"HIP events around single calls, {WARMUP} warm-ups, {args.calls} timed calls, {SETS} sets of fields in rotation; "
        "median [first quartile, third quartile] in microseconds")
    missed, rows = [], 0
    for name, shape, dtype in SHAPES:
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        itemsize = np.dtype(dtype).itemsize
        gen = torch.Generator(device="cuda").manual_seed(1)

        def storage(values=None):
            s = gt_storage.zeros(shape, dtype, backend=backend)
            if values is not None:
                s.tensor.copy_(values)
            return s

        srcs = [[storage(2 * torch.rand(shape, dtype=tdt, device="cuda", generator=gen) - 1) for _ in range(8)] for _ in range(SETS)]
        dsts = [[storage() for _ in range(8)] for _ in range(SETS)]
        stream = torch.cuda.current_stream().cuda_stream
        box = shape[0] * shape[1] * shape[2] * itemsize
        for ax, axis in ((0, "I"), (1, "J")):
            n, nh = shape[ax], shape[ax] // 2 + 1
            others = [d for d in range(3) if d != ax]
            say(f"\n{name}, lines along {axis} (n = {n}, {shape[others[0]] * shape[others[1]]} lines)")
            for count in (1, 8):
                copy = None
                # (a response per index of an axis that the lanes do not run along: J for lines along I, K for lines along J)
                per = (shape[others[0]], 1, nh) if ax == 0 else (1, shape[others[1]], nh)
                for label, rshape in (("shared response", (nh,)), (f"response per {'jk'[ax]}  ", per)):
                    response = torch.rand(rshape, dtype=torch.float64, device="cuda", generator=gen)
                    # the same response as the torch route takes it: wavenumbers along `ax`, in the fields' precision
                    r3 = response.reshape((1, 1, nh) if len(rshape) == 1 else rshape)
                    r_torch = torch.movedim(r3, 2, ax).to(tdt).contiguous()

                    def baseline(s):
                        for f in range(count):
                            torch.fft.irfft(torch.fft.rfft(srcs[s][f].tensor, dim=ax) * r_torch, n=n, dim=ax)

                    frozen = [linefilter.LineFilter(dsts[s][:count], srcs[s][:count], axis=axis, response=response) for s in range(SETS)]
                    assert all(f.launches == 1 for f in frozen)
                    frozen[0]()
                    want = torch.fft.irfft(torch.fft.rfft(srcs[0][0].tensor, dim=ax) * r_torch, n=n, dim=ax)
                    torch.cuda.synchronize()
                    assert torch.allclose(dsts[0][0].tensor, want, rtol=0, atol=1e-3 if dtype is np.float32 else 1e-11), \
                        "the torch route and the kernel disagree"
                    del want
                    algorithmic = 2 * count * box
                    t_a = event_us(baseline, args.calls)
                    if copy is None:
                        half = algorithmic // 2 - (algorithmic // 2) % 16
                        buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
                        copy = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), args.calls)
                        del buf_in, buf_out
                    t_k = event_us(lambda s: frozen[s](), args.calls)
                    met = t_k[1] < t_a[1]
                    rows += 1
                    say(f"  {count} field(s) {label}: (a) torch {show(t_a)}   (b) copy of {algorithmic / 2**20:6.0f} MiB {show(copy)}   "
                        f"(k) LineFilter ({frozen[0].path}) {show(t_k)}   {algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; "
                        f"per field (k) {t_k[1] / count:.1f} (a) {t_a[1] / count:.1f}; (k)/(a) = {t_k[1] / t_a[1]:.3f} {'met' if met else 'MISSED'}, "
                        f"(k)/(b) = {t_k[1] / copy[1]:.3f}")
                    if not met:
                        missed.append(f"{name} along {axis} {count} field(s) {label.strip()}: (k) {t_k[1]:.1f} >= (a) {t_a[1]:.1f}")
                    del frozen, response, r_torch
                    torch.cuda.empty_cache()
        del srcs, dsts
        torch.cuda.empty_cache()
    say(f"\nbar: (k) takes less time than (a) by medians for the same fields -> met in {rows - len(missed)} of {rows} rows"
        + ("" if not missed else "; MISSED: " + "; ".join(missed)))
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
