"""What a vertical interpolation to run-time levels costs (output kept as profiles/vertical_interp_timing.txt).

Per shape (ns source levels to nd target levels), method and number of fields, side by side (HIP events around single calls, 5
warm-ups, 30 timed calls, 3 sets of fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and
quartiles):
  (k) one gt4py_amd.vertical.VerticalInterp call of all the fields (frozen form: one launch per 8 fields), outside="clamp";
  (a) the route a user has without it: the same linear interpolation written as a GTScript stencil on hip:mi300 with
      device_sync=False -- a FORWARD sweep that carries the bracket index in a 2-d temporary, the two `while` loops of the hunt, reads
      at a run-time K index --, called once per field, so the search and the weights are repeated for every field.  If the frontend
      refuses that program the torch formulation is timed instead (searchsorted on the coordinates, gathers, again once per field),
      and the output says so.  The baseline is linear in both cases; it is the reference line for the cubic_monotone rows too (a
      GTScript cubic would cost more).
  (b) gt4mi_stream_copy of the algorithmic bytes: every source item and both coordinate fields in, every target item out.

No bar is fixed in advance: every ratio is reported as measured.  What is expected: the weights are computed once per call instead
of once per field, so (k) for 8 fields should be below (a) for 8 fields; a row that misses that is listed at the end.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/vertical_interp_timing.py, in a run of its own.
"""

from __future__ import annotations

import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from gt4py_amd.cartesian.gtscript import FORWARD, IJ, Field, computation, interval  # noqa: E402,F401

WARMUP = 5
SETS = 3
#: (name, (ni, nj), ns, nd, dtype, numbers of fields)
SHAPES = (("1024x1024, 80 -> 40 levels, float32", (1024, 1024), 80, 40, np.float32, (1, 8)),
          ("512x512, 128 -> 128 levels, float64", (512, 512), 128, 128, np.float64, (1, 8)))


def interp_linear(q: Field["T"], zs: Field["T"], zd: Field["T"], out: Field["T"], *, ns: int):  # noqa: F821
    """The linear method of include/gt4py_amd.h with outside="clamp" as a GTScript stencil for one field (domain = (ni, nj, nd);
    dtypes={"T": ...})."""
    with computation(FORWARD):
        with interval(0, 1):
            ks: Field[IJ, np.int32] = 0
            x = zd
            while ks < ns - 2 and zs.at(K=ks + 1) <= x:
                ks = ks + 1
            while ks > 0 and zs.at(K=ks) > x:
                ks = ks - 1
            x = min(max(x, zs.at(K=0)), zs.at(K=ns - 1))
            zk = zs.at(K=ks)
            t = (x - zk) / (zs.at(K=ks + 1) - zk)
            out = (1.0 - t) * q.at(K=ks) + t * q.at(K=ks + 1)
        with interval(1, None):
            x = zd
            while ks < ns - 2 and zs.at(K=ks + 1) <= x:
                ks = ks + 1
            while ks > 0 and zs.at(K=ks) > x:
                ks = ks - 1
            x = min(max(x, zs.at(K=0)), zs.at(K=ns - 1))
            zk = zs.at(K=ks)
            t = (x - zk) / (zs.at(K=ks + 1) - zk)
            out = (1.0 - t) * q.at(K=ks) + t * q.at(K=ks + 1)


def torch_interp_linear(q, zs, zd):
    """The same interpolation from torch operations: searchsorted for the bracket, gathers for its two levels."""
    import torch

    ns = q.shape[2]
    x = torch.minimum(torch.maximum(zd, zs[..., :1]), zs[..., -1:])
    k = (torch.searchsorted(zs.contiguous(), x.contiguous(), right=True) - 1).clamp_(0, ns - 2)
    zk, zk1 = torch.gather(zs, 2, k), torch.gather(zs, 2, k + 1)
    t = (x - zk) / (zk1 - zk)
    return (1.0 - t) * torch.gather(q, 2, k) + t * torch.gather(q, 2, k + 1)


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vertical_interp_timing.txt"))
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, vertical
    from gt4py_amd.cartesian import gtscript

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
    for name, (ni, nj), ns, nd, dtype, counts in SHAPES:
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        itemsize = np.dtype(dtype).itemsize
        gen = torch.Generator(device="cuda").manual_seed(1)
        most = max(counts)

        def storage(levels, values):
            s = gt_storage.zeros((ni, nj, levels), dtype, backend=backend)
            s.tensor.copy_(values)
            return s

        def source_coord():  # increasing along K, different in every column (ln p of a terrain-following model)
            inc = 0.5 + torch.rand((ni, nj, ns), dtype=torch.float64, device="cuda", generator=gen)
            return torch.cumsum(inc, dim=2).to(tdt)

        def target_coord(zs):  # increasing levels per column that reach a little outside the source range at both ends
            lo, hi = zs[..., :1].double() - 1.0, zs[..., -1:].double() + 1.0
            inc = 0.5 + torch.rand((ni, nj, nd), dtype=torch.float64, device="cuda", generator=gen)
            t = torch.cumsum(inc, dim=2)
            return (lo + (hi - lo) * (t - t[..., :1]) / (t[..., -1:] - t[..., :1])).to(tdt)

        zs = [storage(ns, source_coord()) for _ in range(SETS)]
        zd = [storage(nd, target_coord(z.tensor)) for z in zs]
        srcs = [[storage(ns, torch.rand((ni, nj, ns), dtype=tdt, device="cuda", generator=gen)) for _ in range(most)] for _ in range(SETS)]
        dsts = [[gt_storage.zeros((ni, nj, nd), dtype, backend=backend) for _ in range(most)] for _ in range(SETS)]
        check = gt_storage.zeros((ni, nj, nd), dtype, backend=backend)
        # (a): GTScript if the frontend takes the program, else torch
        try:
            stencil = gtscript.stencil(backend=backend, definition=interp_linear, dtypes={"T": dtype}, device_sync=False, while_loops="pointwise")
            stencil(srcs[0][0], zs[0], zd[0], check, ns=ns, origin=(0, 0, 0), domain=(ni, nj, nd))
            torch.cuda.synchronize()
            route_a = "GTScript stencil (FORWARD, carried index, two while loops, run-time K reads), once per field"

            def baseline(s, count):
                for n in range(count):
                    stencil(srcs[s][n], zs[s], zd[s], dsts[s][n], ns=ns, origin=(0, 0, 0), domain=(ni, nj, nd))
        except Exception as exc:  # noqa: BLE001 - whatever the frontend or the code generator refuses
            say(f"  (the frontend refused the GTScript interpolation: {type(exc).__name__}: {str(exc)[:200]})")
            route_a = "torch formulation (searchsorted + gathers), once per field"
            check.tensor.copy_(torch_interp_linear(srcs[0][0].tensor, zs[0].tensor, zd[0].tensor))

            def baseline(s, count):
                for n in range(count):
                    dsts[s][n].tensor.copy_(torch_interp_linear(srcs[s][n].tensor, zs[s].tensor, zd[s].tensor))
        # the same numbers? (the same formula; the stencil's arithmetic is in the fields' dtype: within rounding)
        vertical.interpolate_levels(dsts[0][0], srcs[0][0], src_coord=zs[0], dst_coord=zd[0], method="linear", outside="clamp")
        torch.cuda.synchronize()
        tol = 1e-4 if dtype is np.float32 else 1e-11
        assert torch.allclose(dsts[0][0].tensor, check.tensor, rtol=tol, atol=tol), "the baseline and the kernel disagree"
        say(f"\n{name}: (a) = {route_a}")
        stream = torch.cuda.current_stream().cuda_stream
        for count in counts:
            algorithmic = (count * ni * nj * (ns + nd) + ni * nj * (ns + nd)) * itemsize
            t_a = event_us(lambda s: baseline(s, count), args.calls)
            say(f"  {count} field(s): (a) baseline, linear, {count} call(s)                       {show(t_a)}")
            half = algorithmic // 2 - (algorithmic // 2) % 16
            buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
            t_b = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), args.calls)
            say(f"  {count} field(s): (b) gt4mi_stream_copy, {algorithmic / 2**20:6.0f} MiB in + out           {show(t_b)}")
            del buf_in, buf_out
            for method in ("linear", "cubic_monotone"):
                frozen = [vertical.VerticalInterp(dsts[s][:count], srcs[s][:count], src_coord=zs[s], dst_coord=zd[s], method=method)
                          for s in range(SETS)]
                assert all(f.launches == 1 for f in frozen)
                t_k = event_us(lambda s: frozen[s](), args.calls)
                say(f"  {count} field(s): (k) VerticalInterp {method:14s}, one launch        {show(t_k)}   "
                    f"{algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; (k)/(a) = {t_k[1] / t_a[1]:.3f}, (k)/(b) = {t_k[1] / t_b[1]:.3f}")
                if t_k[1] > t_a[1]:
                    missed.append(f"{name} {count} field(s) {method}: (k) {t_k[1]:.1f} > (a) {t_a[1]:.1f}")
        del zs, zd, srcs, dsts, check
        torch.cuda.empty_cache()
    say(f"\nexpected: (k) <= (a) by medians for the same fields -> {'seen in every row' if not missed else 'NOT seen in: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
