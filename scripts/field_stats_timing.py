"""What the statistics of a field cost (output kept as profiles/field_stats_timing.txt).

Per configuration, side by side (HIP events, 5 warm-ups, 40 timed calls, rotating over enough fields that the Infinity Cache does
not serve repeats -- BASELINE.md section 4):
  1. one gt4py_amd.diagnostics.FieldStats call of one field (frozen form: the pass and the finishing launch);
  2. the route there was before: the six torch reductions on the same domain view (sum, abs().sum, (x*x).sum, min, max, isfinite
     count), left on the device without .item() -- the fairest form of it;
  3. gt4mi_stream_copy of the field's byte span: the same bytes in AND out;
  4. 8 fields in one call against 8 calls of one field.

Acceptance: (1) <= (2) -- one pass must not lose to six -- and (1) <= (3) -- a read-once pass slower than reading and writing
the same bytes is not streaming.  Both bars are code that is not under test, so they carry no margin beyond the run-to-run spread
the mean and median columns show; the script exits non-zero when a bar is missed (means compared).
Every timed window is ONE call under its own event pair: call-to-call figures that include the launches.
Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/field_stats_timing.py (profiles/field_stats_rocprofv3_kernel_stats.csv).

    python scripts/field_stats_timing.py [--calls 40]
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

WARMUP = 5
HBM_PEAK = 8.0e12  # bytes per second


def event_ms(fn, calls, nfields):
    """Mean and median time of fn(n) over `calls` calls, n rotating over the fields; one event pair around each call."""
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


def torch_route(view):
    """Six reductions, results left on the device."""
    import torch

    return (view.sum(), view.abs().sum(), (view * view).sum(), view.min(), view.max(), torch.isfinite(view).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, diagnostics

    backend = "hip:mi300"
    lib = _lib.load()
    print(_lib.device_info())
    print(f"HIP events, {WARMUP} warm-ups, {args.calls} timed calls; mean (median) in microseconds")
    missed = []
    for name, domain, dtype, w in (("512x512x512 float64, halo 1", (512, 512, 512), np.float64, 1),
                                   ("1024x1024x80 float32, halo 2", (1024, 1024, 80), np.float32, 2)):
        shape = (domain[0] + 2 * w, domain[1] + 2 * w, domain[2])
        itemsize = np.dtype(dtype).itemsize
        nbytes = int(np.prod(shape)) * itemsize
        domain_bytes = int(np.prod(domain)) * itemsize
        nfields = max(8, int(np.ceil(1.5 * 2**30 / nbytes)))  # > 1 GiB in rotation: 4x the 256 MiB Infinity Cache; 8 for (4)
        fields = [gt_storage.zeros(shape, dtype, backend=backend, aligned_index=(w, w, 0)) for _ in range(nfields)]
        gen = torch.Generator(device="cuda").manual_seed(1)
        for f in fields:
            f.tensor.copy_(torch.rand(shape, dtype=f.tensor.dtype, device="cuda", generator=gen))
        views = [f.tensor[w:-w, w:-w] for f in fields]
        frozen = [diagnostics.FieldStats([f], halo=w) for f in fields]
        assert all(f.launches == 2 for f in frozen)
        t_one = event_ms(lambda n: frozen[n](), args.calls, nfields)
        t_torch = event_ms(lambda n: torch_route(views[n]), args.calls, nfields)
        # the byte span of the field's domain: first to last point, rounded to 16-byte lanes
        f0 = fields[0]
        stride = f0.strides
        span = (domain[0] - 1) * stride[0] + (domain[1] - 1) * stride[1] + (domain[2] - 1) * stride[2] + itemsize
        span -= span % 16
        dst = torch.empty(span, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        starts = [f.ptr + (-f.ptr) % 16 for f in fields]
        t_copy = event_ms(lambda n: lib.gt4mi_stream_copy(starts[n], dst.data_ptr(), span, stream), args.calls, nfields)
        # same numbers? sum against torch within the rounding of two different orders; count and extremes exactly
        frozen[0]()
        s, = frozen[0].get()
        ref = [float(v) for v in torch_route(views[0])]
        assert s.count == views[0].numel() and s.nonfinite == views[0].numel() - ref[5] and (s.min, s.max) == (ref[3], ref[4])
        assert abs(s.sum - ref[0]) <= 1e-4 * ref[1] and abs(s.sum_sq - ref[2]) <= 1e-4 * ref[2]
        groups = nfields // 8
        eight = [diagnostics.FieldStats(fields[8 * g: 8 * g + 8], halo=w) for g in range(groups)]
        assert all(e.launches == 2 for e in eight)
        t_eight = event_ms(lambda n: eight[n](), args.calls, groups)

        def eight_calls(n):
            for f in frozen[8 * n: 8 * n + 8]:
                f()

        t_eight_calls = event_ms(eight_calls, args.calls, groups)
        rate = domain_bytes / (t_one[0] * 1e-3)
        rate8 = 8 * domain_bytes / (t_eight[0] * 1e-3)
        print(f"\n{name}: {nfields} fields of {nbytes / 2**20:.0f} MiB in rotation, {domain_bytes / 2**20:.0f} MiB of domain per field")
        print(f"  (1) FieldStats, one field (2 launches)        {t_one[0] * 1e3:9.1f} ({t_one[1] * 1e3:.1f})   "
              f"reads {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak")
        print(f"  (2) six torch reductions on the domain view   {t_torch[0] * 1e3:9.1f} ({t_torch[1] * 1e3:.1f})   (1) / (2) = {t_one[0] / t_torch[0]:.3f}")
        print(f"  (3) gt4mi_stream_copy of the byte span        {t_copy[0] * 1e3:9.1f} ({t_copy[1] * 1e3:.1f})   (1) / (3) = {t_one[0] / t_copy[0]:.3f}"
              f"   ({2 * span / (t_copy[0] * 1e-3) / 1e12:.2f} TB/s in + out)")
        print(f"  (4) 8 fields in one call (2 launches)         {t_eight[0] * 1e3:9.1f} ({t_eight[1] * 1e3:.1f})   "
              f"reads {rate8 / 1e12:.2f} TB/s = {100 * rate8 / HBM_PEAK:.0f} % of the peak")
        print(f"      8 calls of one field (16 launches)        {t_eight_calls[0] * 1e3:9.1f} ({t_eight_calls[1] * 1e3:.1f})   "
              f"one call / eight calls = {t_eight[0] / t_eight_calls[0]:.3f}")
        if t_one[0] > t_torch[0]:
            missed.append(f"{name}: (1) > (2)")
        if t_one[0] > t_copy[0]:
            missed.append(f"{name}: (1) > (3)")
        del fields, views, frozen, eight, dst
        torch.cuda.empty_cache()
    print(f"\nacceptance: (1) <= (2) and (1) <= (3) in every configuration -> {'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
