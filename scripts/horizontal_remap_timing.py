"""What a conservative horizontal remapping costs (output kept as profiles/horizontal_remap_timing.txt).

Per case, number of fields (1 and 8) and method, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3 sets
of fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.horizontal.HorizontalRemap call of all the fields (frozen form: one launch per 8 fields);
  (a) the torch routes a user has without it, on the same tensors, once per field:
      (a1) two dense weight-matrix products (the pcm weights of the two overlap tables as nd x ns matrices; einsum along I, then
           along J) and a copy into dst;
      (a2) torch.nn.functional.avg_pool2d on a permuted view, where the grids are uniform and the ratio is 2:1;
      torch has no counterpart of plm: its rows are set against the same (a1) / (a2), which compute less;
  (b) gt4mi_stream_copy of the algorithmic bytes: src + dst per field.

Cases: 1024x1024x80 float32 -> 512x512 (uniform 2:1) and -> 341x384 (a non-integer ratio, irregular edges), 512x512x128 float64 ->
1024x1024 (uniform 1:2 refinement).

Bar: (k) <= (a1) and, where it exists, (k) <= (a2) by medians for the same fields, with disjoint quartile ranges.  The script
exits non-zero when the bar is missed.  (k)/(b) is reported as measured and carries no bar.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/horizontal_remap_timing.py, in a run of its own.
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


def irregular(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, n))])
    x = lo + (hi - lo) * t / t[-1]
    x[0], x[-1] = lo, hi
    return x


CASES = (
    ("1024x1024x80 float32 -> 512x512 (uniform 2:1)", (1024, 1024, 80), np.float32,
     (np.arange(1025.0), np.arange(1025.0)), (np.arange(513.0) * 2, np.arange(513.0) * 2), True),
    ("1024x1024x80 float32 -> 341x384 (irregular edges)", (1024, 1024, 80), np.float32,
     (irregular(1024, 0.0, 1024.0, 1), irregular(1024, 0.0, 1024.0, 2)), (irregular(341, 0.0, 1024.0, 3), irregular(384, 0.0, 1024.0, 4)), False),
    ("512x512x128 float64 -> 1024x1024 (uniform 1:2)", (512, 512, 128), np.float64,
     (np.arange(513.0) * 2, np.arange(513.0) * 2), (np.arange(1025.0), np.arange(1025.0)), False),
)


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


def dense_weights(horizontal, xs, xd, tdt):
    """The pcm weights of one axis as an nd x ns matrix on the device."""
    import torch

    ptr, cell, w, *_ = horizontal.overlap_table(xs, xd)
    m = np.zeros((xd.size - 1, xs.size - 1))
    m[np.repeat(np.arange(xd.size - 1), np.diff(ptr)), cell] = w
    return torch.from_numpy(m).to(device="cuda", dtype=tdt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "horizontal_remap_timing.txt"))
    args = ap.parse_args()
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, horizontal

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
    for name, s_shape, dtype, xs, xd, pool in CASES:
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        itemsize = np.dtype(dtype).itemsize
        gen = torch.Generator(device="cuda").manual_seed(1)
        d_shape = (xd[0].size - 1, xd[1].size - 1, s_shape[2])

        def storage(shape, values=None):
            s = gt_storage.zeros(shape, dtype, backend=backend)
            if values is not None:
                s.tensor.copy_(values)
            return s

        srcs = [[storage(s_shape, torch.rand(s_shape, dtype=tdt, device="cuda", generator=gen)) for _ in range(8)] for _ in range(SETS)]
        dsts = [[storage(d_shape) for _ in range(8)] for _ in range(SETS)]
        check = storage(d_shape)
        w_i, w_j = dense_weights(horizontal, xs[0], xd[0], tdt), dense_weights(horizontal, xs[1], xd[1], tdt)

        def matrix_route(s, count):
            for n in range(count):
                rows = torch.einsum("ma,abk->mbk", w_i, srcs[s][n].tensor)
                dsts[s][n].tensor.copy_(torch.einsum("nb,mbk->mnk", w_j, rows))

        def pool_route(s, count):
            for n in range(count):
                out = torch.nn.functional.avg_pool2d(srcs[s][n].tensor.permute(2, 0, 1).unsqueeze(0), 2)
                dsts[s][n].tensor.copy_(out[0].permute(1, 2, 0))

        # the same numbers?  A sanity check, not the contract: torch orders the additions its own way, in the fields' dtype
        tol = 1e-5 if dtype is np.float32 else 1e-13
        horizontal.remap_cells(check, srcs[0][0], src_edges=xs, dst_edges=xd)
        for route in (matrix_route, pool_route) if pool else (matrix_route,):
            route(0, 1)
            torch.cuda.synchronize()
            worst = float((dsts[0][0].tensor - check.tensor).abs().max())
            assert worst <= tol, f"{route.__name__} and the kernel disagree: {worst}"
        say(f"\n{name}")
        stream = torch.cuda.current_stream().cuda_stream
        for count in (1, 8):
            algorithmic = count * (int(np.prod(s_shape)) + int(np.prod(d_shape))) * itemsize
            half = algorithmic // 2 - (algorithmic // 2) % 16
            buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
            t_b = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), args.calls)
            say(f"  {count} field(s): (b) gt4mi_stream_copy, {algorithmic / 2**20:6.0f} MiB in + out      {show(t_b)}")
            del buf_in, buf_out
            against = [("(a1) torch, two weight-matrix products", event_us(lambda s: matrix_route(s, count), args.calls))]
            if pool:
                against.append(("(a2) torch avg_pool2d", event_us(lambda s: pool_route(s, count), args.calls)))
            for what, t in against:
                say(f"  {count} field(s): {what:<42} {show(t)}")
            for method in ("pcm", "plm"):
                frozen = [horizontal.HorizontalRemap(dsts[s][:count], srcs[s][:count], src_edges=xs, dst_edges=xd, method=method) for s in range(SETS)]
                assert all(f.launches == 1 for f in frozen)
                t_k = event_us(lambda s: frozen[s](), args.calls)
                ratios = ", ".join(f"(k)/{what[:4]} = {t_k[1] / t[1]:.3f} (quartiles {'disjoint' if t_k[2] < t[0] or t[2] < t_k[0] else 'overlap'})"
                                   for what, t in against)
                say(f"  {count} field(s): (k) HorizontalRemap {method}, one launch        {show(t_k)}   "
                    f"{algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; {ratios}, (k)/(b) = {t_k[1] / t_b[1]:.2f}")
                for what, t in against:
                    if not t_k[2] < t[0]:
                        missed.append(f"{name} {count} field(s) {method}: (k) {show(t_k).strip()} against {what[:4]} {show(t).strip()}")
        del srcs, dsts, check
        torch.cuda.empty_cache()
    say(f"\nbar: (k) faster than (a1) and (a2) by medians with disjoint quartiles for the same fields -> "
        f"{'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
