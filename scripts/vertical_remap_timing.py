"""What a conservative vertical remap costs (output kept as profiles/vertical_remap_timing.txt).

Per shape (ns = nd), method and number of fields, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3
sets of fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.vertical.VerticalRemap call of all the fields (frozen form: one launch per 8 fields);
  (a) the route a user has without it: the same PCM remap written as a GTScript stencil on hip:mi300 with device_sync=False -- a
      FORWARD sweep that carries the source index in a 2-d temporary, a `while` over the overlapping source cells, reads at a
      run-time K index --, called once per field.  If the frontend refuses that program the torch formulation is timed instead
      (searchsorted on the edges, gathers from the cumulative column integral, again once per field), and the output says so.
      The baseline is PCM in both cases; it is the reference line for the PLM rows too (GTScript PLM would cost more).
  (b) gt4mi_stream_copy of the algorithmic bytes: every source item and both edge fields in, every target item out.

Bar: (k) <= (a) by medians for the same fields, no margin beyond the quartiles printed; the script exits non-zero when it is
missed.  (k)/(b) is reported and carries no bar.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/vertical_remap_timing.py, in a run of its own.
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
SHAPES = (("1024x1024x80 float32", (1024, 1024, 80), np.float32),
          ("512x512x128 float64", (512, 512, 128), np.float64))


def remap_pcm(q: Field["T"], zs: Field["T"], zd: Field["T"], out: Field["T"], *, ns: int):  # noqa: F821
    """The PCM remap of include/gt4py_amd.h as a GTScript stencil for one field (domain = (ni, nj, nd); dtypes={"T": ...})."""
    with computation(FORWARD):
        with interval(0, 1):
            ks: Field[IJ, np.int32] = 0
            lo = zd
            hi = zd[0, 0, 1]
            while ks < ns - 1 and zs.at(K=ks + 1) <= lo:
                ks = ks + 1
            acc = 0.0
            more = 1
            while more == 1:
                zk = zs.at(K=ks)
                zk1 = zs.at(K=ks + 1)
                left = lo if ks == 0 else max(lo, zk)
                right = hi if ks == ns - 1 else min(hi, zk1)
                acc = acc + (right - left) / (hi - lo) * q.at(K=ks)
                if ks == ns - 1 or zk1 >= hi:
                    more = 0
                else:
                    ks = ks + 1
            out = acc
        with interval(1, None):
            lo = zd
            hi = zd[0, 0, 1]
            while ks < ns - 1 and zs.at(K=ks + 1) <= lo:
                ks = ks + 1
            acc = 0.0
            more = 1
            while more == 1:
                zk = zs.at(K=ks)
                zk1 = zs.at(K=ks + 1)
                left = lo if ks == 0 else max(lo, zk)
                right = hi if ks == ns - 1 else min(hi, zk1)
                acc = acc + (right - left) / (hi - lo) * q.at(K=ks)
                if ks == ns - 1 or zk1 >= hi:
                    more = 0
                else:
                    ks = ks + 1
            out = acc


def torch_remap_pcm(q, zs, zd):
    """The PCM remap from torch operations: the cumulative column integral read at the target edges (searchsorted + gathers); the
    end cells extend linearly, which is the constant extension of their means."""
    import torch

    ns = q.shape[2]
    dz = zs[..., 1:] - zs[..., :-1]
    cum = torch.cumsum(q * dz, dim=2) - q * dz  # integral up to the cell's lower edge
    k = (torch.searchsorted(zs.contiguous(), zd.contiguous(), right=True) - 1).clamp_(0, ns - 1)
    integral = torch.gather(cum, 2, k) + torch.gather(q, 2, k) * (zd - torch.gather(zs, 2, k))
    return (integral[..., 1:] - integral[..., :-1]) / (zd[..., 1:] - zd[..., :-1])


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vertical_remap_timing.txt"))
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
    for name, (ni, nj, nk), dtype in SHAPES:
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        itemsize = np.dtype(dtype).itemsize
        gen = torch.Generator(device="cuda").manual_seed(1)

        def storage(levels, values):
            s = gt_storage.zeros((ni, nj, levels), dtype, backend=backend)
            s.tensor.copy_(values)
            return s

        def edges():  # increasing along K, different in every column
            inc = 0.5 + torch.rand((ni, nj, nk + 1), dtype=torch.float64, device="cuda", generator=gen)
            return torch.cumsum(inc, dim=2).to(tdt)

        # one pair of edge fields per set (a model's moving levels -> its output levels), 8 sources and 8 destinations per set
        zs = [storage(nk + 1, edges()) for _ in range(SETS)]
        zd = [storage(nk + 1, edges()) for _ in range(SETS)]
        srcs = [[storage(nk, torch.rand((ni, nj, nk), dtype=tdt, device="cuda", generator=gen)) for _ in range(8)] for _ in range(SETS)]
        dsts = [[gt_storage.zeros((ni, nj, nk), dtype, backend=backend) for _ in range(8)] for _ in range(SETS)]
        check = gt_storage.zeros((ni, nj, nk), dtype, backend=backend)
        # (a): GTScript if the frontend takes the program, else torch
        try:
            stencil = gtscript.stencil(backend=backend, definition=remap_pcm, dtypes={"T": dtype}, device_sync=False, while_loops="pointwise")
            stencil(srcs[0][0], zs[0], zd[0], check, ns=nk)
            torch.cuda.synchronize()
            route_a = "GTScript stencil (FORWARD, carried index, while, run-time K reads), once per field"

            def baseline(s, count):
                for n in range(count):
                    stencil(srcs[s][n], zs[s], zd[s], dsts[s][n], ns=nk)
        except Exception as exc:  # noqa: BLE001 - whatever the frontend or the code generator refuses
            say(f"  (the frontend refused the GTScript remap: {type(exc).__name__}: {str(exc)[:200]})")
            route_a = "torch formulation (searchsorted + gathers), once per field"
            check.tensor.copy_(torch_remap_pcm(srcs[0][0].tensor, zs[0].tensor, zd[0].tensor))

            def baseline(s, count):
                for n in range(count):
                    dsts[s][n].tensor.copy_(torch_remap_pcm(srcs[s][n].tensor, zs[s].tensor, zd[s].tensor))
        # the same numbers? (two orders of the same sum: within rounding)
        vertical.remap_levels(dsts[0][0], srcs[0][0], src_edges=zs[0], dst_edges=zd[0], method="pcm")
        torch.cuda.synchronize()
        tol = 1e-4 if dtype is np.float32 else 1e-11
        assert torch.allclose(dsts[0][0].tensor, check.tensor, rtol=tol, atol=tol), "the baseline and the kernel disagree"
        say(f"\n{name}, ns = nd = {nk}: (a) = {route_a}")
        stream = torch.cuda.current_stream().cuda_stream
        for count in (1, 8):
            algorithmic = (2 * count * ni * nj * nk + 2 * ni * nj * (nk + 1)) * itemsize
            t_a = event_us(lambda s: baseline(s, count), args.calls)
            say(f"  {count} field(s): (a) baseline, PCM                         {show(t_a)}")
            half = algorithmic // 2 - (algorithmic // 2) % 16
            buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
            t_b = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), args.calls)
            say(f"  {count} field(s): (b) gt4mi_stream_copy, {algorithmic / 2**20:6.0f} MiB in + out  {show(t_b)}")
            del buf_in, buf_out
            for method in ("pcm", "plm"):
                frozen = [vertical.VerticalRemap(dsts[s][:count], srcs[s][:count], src_edges=zs[s], dst_edges=zd[s], method=method)
                          for s in range(SETS)]
                assert all(f.launches == 1 for f in frozen)
                t_k = event_us(lambda s: frozen[s](), args.calls)
                say(f"  {count} field(s): (k) VerticalRemap {method}, one launch           {show(t_k)}   "
                    f"{algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; (k)/(a) = {t_k[1] / t_a[1]:.3f}, (k)/(b) = {t_k[1] / t_b[1]:.3f}")
                if t_k[1] > t_a[1]:
                    missed.append(f"{name} {count} field(s) {method}: (k) {t_k[1]:.1f} > (a) {t_a[1]:.1f}")
        del zs, zd, srcs, dsts, check
        torch.cuda.empty_cache()
    say(f"\nbar: (k) <= (a) by medians for the same fields -> {'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
