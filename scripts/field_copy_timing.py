"""What moving a field between the storage layout and numpy's C order costs (output kept as profiles/field_copy_timing.txt).

Per configuration (512^3 float64 and 1024^2 x 80 float32, the BASELINE-size fields), side by side -- HIP events around single
calls, 5 warm-ups, medians of 40 timed calls, 8 pairs of buffers in rotation so that the Infinity Cache does not serve repeats:
  (a) gt4py_amd.transfer.FieldCopy, the tile path: storage layout (I-contiguous, padded rows) -> C order (K fastest), and back;
  (b) torch's copy_ on the very same two views: the route there was before;
  (c) gt4mi_stream_copy of the same bytes: the floor;
  (d) end to end on the host's clock, the device idle before and after: transfer.Download + get() against DeviceArray.get(),
      and transfer.Upload against storage[...] = host.

The bar is the former route, never the new code itself: (a) <= (b) in both directions and Download + get() <= DeviceArray.get(),
medians compared, with no margin beyond the spread (the quartiles printed next to every figure).  (a) / (c) is reported without
a bar.  Each configuration runs in a child process of its own under a time limit; the first one that fails ends the script.

    python scripts/field_copy_timing.py [--calls 40] [--output profiles/field_copy_timing.txt]
"""

from __future__ import annotations

import argparse
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WARMUP = 5
ROTATION = 8
CONFIGS = (("512x512x512 float64, halo 1", (512, 512, 512), "float64", 1),
           ("1024x1024x80 float32, halo 2", (1024, 1024, 80), "float32", 2))
CHILD_TIMEOUT = 420  # seconds per configuration


class Times:
    def __init__(self, ms):
        ms = sorted(ms)
        self.median, self.lo, self.hi = ms[len(ms) // 2], ms[len(ms) // 4], ms[(3 * len(ms)) // 4]

    def __str__(self):
        return f"{self.median * 1e3:10.1f} us  (quartiles {self.lo * 1e3:.1f} .. {self.hi * 1e3:.1f})"


def ratio(a: Times, b: Times) -> str:
    """Ratio of the medians, and the range the quartiles of both leave it."""
    return f"{a.median / b.median:.3f}  (spread {a.lo / b.hi:.3f} .. {a.hi / b.lo:.3f})"


def verdict(a: Times, b: Times) -> str:
    if a.median <= b.median:
        return "met"
    return "NOT met, though inside the spread" if a.lo <= b.hi else "NOT met"


def event_ms(fn, calls) -> Times:
    """fn(n) under an event pair of its own, n rotating over the buffers."""
    import torch

    for n in range(WARMUP):
        fn(n % ROTATION)
    torch.cuda.synchronize()
    pairs = []
    for c in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn(c % ROTATION)
        stop.record()
        pairs.append((start, stop))
    torch.cuda.synchronize()
    return Times([a.elapsed_time(b) for a, b in pairs])


def wall_ms(fn, calls) -> Times:
    """fn(n) on the host's clock, the device idle before it starts; fn returns when its result is usable."""
    import torch

    times = []
    for c in range(2 + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(c % ROTATION)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return Times(times[2:])


def run_config(index: int, calls: int) -> int:
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, transfer

    name, domain, dtype, w = CONFIGS[index]
    dtype = np.dtype(dtype)
    lib = _lib.load()
    if index == 0:
        print(_lib.device_info())
        print(f"HIP events around single calls, {WARMUP} warm-ups, medians of {calls} timed calls, {ROTATION} pairs of buffers in rotation")
    shape = (domain[0] + 2 * w, domain[1] + 2 * w, domain[2])
    nbytes = int(np.prod(shape)) * dtype.itemsize
    tdt = {"float64": torch.float64, "float32": torch.float32}[dtype.name]
    gen = torch.Generator(device="cuda").manual_seed(1)
    fields = [gt_storage.empty(shape, dtype, backend="hip:mi300", aligned_index=(w, w, 0)) for _ in range(ROTATION)]
    dense = [torch.empty(shape, dtype=tdt, device="cuda") for _ in range(ROTATION)]  # numpy's C order
    for f, d in zip(fields, dense):
        d.copy_(torch.rand(shape, dtype=tdt, device="cuda", generator=gen))
        f.tensor.copy_(d)
    views = [f.tensor for f in fields]
    out = [transfer.FieldCopy(d, f, halo=w) for d, f in zip(dense, fields)]
    back = [transfer.FieldCopy(f, d, halo=w) for d, f in zip(dense, fields)]
    assert all(c.paths == [transfer.PATH_TILES] and c.launches == 1 and c.extent == shape for c in out + back)
    # the same bits as the former route, both ways
    check = torch.empty_like(dense[0])
    check.copy_(views[1])
    transfer.copy_fields(dense[0], fields[1], halo=w)
    assert torch.equal(dense[0], check)
    transfer.copy_fields(fields[0], dense[0], halo=w)
    assert torch.equal(views[0], views[1])
    del check

    a_out = event_ms(lambda n: out[n](), calls)
    b_out = event_ms(lambda n: dense[n].copy_(views[n]), calls)
    a_back = event_ms(lambda n: back[n](), calls)
    b_back = event_ms(lambda n: views[n].copy_(dense[n]), calls)
    span = nbytes - nbytes % 16
    stream = torch.cuda.current_stream().cuda_stream
    floor = [torch.empty(span, dtype=torch.uint8, device="cuda") for _ in range(2)]
    c_copy = event_ms(lambda n: lib.gt4mi_stream_copy(dense[n].data_ptr(), floor[n % 2].data_ptr(), span, stream), calls)
    del floor
    print(f"\n{name}: arrays of {shape}, {nbytes / 2**20:.0f} MiB each")
    for what, a, b in (("storage layout -> C order", a_out, b_out), ("C order -> storage layout", a_back, b_back)):
        rate = 2 * nbytes / (a.median * 1e-3)
        print(f"  {what}")
        print(f"    (a) FieldCopy, tile path, one launch   {a}   {rate / 1e12:.2f} TB/s in + out")
        print(f"    (b) torch copy_ on the same two views  {b}   (a) / (b) = {ratio(a, b)}   bar (a) <= (b): {verdict(a, b)}")
        print(f"    (c) gt4mi_stream_copy of the bytes     {c_copy}   (a) / (c) = {ratio(a, c_copy)}")
    missed = [what for what, a, b in (("out", a_out, b_out), ("back", a_back, b_back)) if a.median > b.median]

    # (d) end to end
    host_calls = max(8, calls // 4) if nbytes > 2**29 else calls
    downs = [transfer.Download([f]) for f in fields[:2]]
    d_new = wall_ms(lambda n: downs[n % 2]().get(), host_calls)
    d_old = wall_ms(lambda n: fields[n].get(), host_calls)
    got, = downs[0]().get()
    assert np.array_equal(got, fields[0].get())
    del downs
    host = [np.ascontiguousarray(got), np.ascontiguousarray(got[::-1])]
    ups = [transfer.Upload([f]) for f in fields[:2]]

    def old_upload(n):
        fields[n][...] = host[n % 2]

    u_new = wall_ms(lambda n: ups[n % 2]([host[n % 2]]), host_calls)
    u_old = wall_ms(old_upload, host_calls)
    print(f"  device -> host, on the host's clock ({host_calls} calls)")
    print(f"    (d) Download()() + get(): pinned, C order {d_new}")
    print(f"        DeviceArray.get()                     {d_old}   ratio {ratio(d_new, d_old)}   bar Download <= get(): {verdict(d_new, d_old)}")
    print("  host -> device")
    print(f"    (d) Upload()(host)                        {u_new}")
    print(f"        storage[...] = host                   {u_old}   ratio {ratio(u_new, u_old)}   (no bar)")
    if d_new.median > d_old.median:
        missed.append("download")
    print(f"  bars of this configuration: {'all met' if not missed else 'MISSED: ' + ', '.join(missed)}")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--config", type=int, default=None, help="run one configuration in this process (what the script does per child)")
    ap.add_argument("--output", default=str(ROOT / "profiles" / "field_copy_timing.txt"))
    args = ap.parse_args()
    if args.config is not None:
        return run_config(args.config, args.calls)
    text = []
    for index in range(len(CONFIGS)):
        try:
            child = subprocess.run([sys.executable, __file__, "--config", str(index), "--calls", str(args.calls)], timeout=CHILD_TIMEOUT,
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired as exc:
            print(exc.stdout or "", flush=True)
            print(f"configuration {index} ran into its time limit of {CHILD_TIMEOUT} s: stopping")
            return 124
        print(child.stdout, end="", flush=True)
        if child.returncode != 0:
            print(f"configuration {index} ended with status {child.returncode}: stopping")
            return child.returncode
        text.append(child.stdout)
    out = pathlib.Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
