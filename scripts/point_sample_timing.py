"""What sampling fields at a list of points costs (output kept as profiles/point_sample_timing.txt).

Per shape, number of fields (1 and 8), number of points (1 000 and 100 000) and method, side by side (HIP events around single
calls, 5 warm-ups, 30 timed calls, 3 sets of fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median
and quartiles):
  (k) one gt4py_amd.sampling.Sample call of all the fields (frozen form: one launch per 8 fields), float64 positions drawn
      uniformly over the compute domain -- scattered stations, every point a column of its own: column mode `nearest`, `linear`
      and `cubic_monotone`, point mode `linear`;
  (a) today's device route, torch advanced indexing once per field, the integer indices and the weights computed ONCE outside
      the timed region: `t[ii, jj, :]` for `nearest`; four such gathers and their weights for column-mode `linear`; eight
      gathers `t[ii, jj, kk]` for point-mode `linear`; each call makes fresh tensors, as that route does.  torch has no
      counterpart of `cubic_monotone`: that row has no (a);
  (b) gt4mi_stream_copy of the result's bytes.

Bar: every row that has an (a): (k) <= (a) by medians with disjoint quartile ranges.  The script exits non-zero when a row misses
it.  (k)/(b) is recorded and carries no bar: the work is a latency-bound gather, not a stream, and no roofline fraction is claimed.

Every shape is measured in a child process of its own under a time limit; the parent opens no device, stops at the first child
that fails and writes what was measured so far.
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
HALO = 3
STEP_TIMEOUT = 420  # seconds for one shape
SHAPES = (("1024x1024x80 float32", (1024, 1024, 80), np.float32),
          ("512x512x128 float64", (512, 512, 128), np.float64))
POINTS = (1_000, 100_000)
ROWS = (("column", "nearest"), ("column", "linear"), ("column", "cubic_monotone"), ("point", "linear"))
BAR = "bar: every row with an (a): (k) <= (a) by medians with disjoint quartiles"


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
    return f"{t[1]:9.1f}  [{t[0]:.1f}, {t[2]:.1f}]"


def measure(step: int, calls: int) -> int:
    """One shape, in this process; prints the lines of the profile.  Returns 1 when a row misses the bar."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, sampling

    say = lambda text="": print(text, flush=True)  # noqa: E731
    backend = "hip:mi300"
    lib = _lib.load()
    name, shape, dtype = SHAPES[step]
    tdt = torch.float32 if dtype is np.float32 else torch.float64
    itemsize = np.dtype(dtype).itemsize
    gen = torch.Generator(device="cuda").manual_seed(1)
    ni, nj, nk = shape[0] - 2 * HALO, shape[1] - 2 * HALO, shape[2]
    origin = (HALO, HALO, 0)

    def storage():
        s = gt_storage.zeros(shape, dtype, backend=backend, aligned_index=origin)
        s.tensor.copy_(torch.rand(shape, dtype=tdt, device="cuda", generator=gen))
        return s

    fields = [[storage() for _ in range(8)] for _ in range(SETS)]
    say(f"\n{name} arrays, halo {HALO}, domain {ni}x{nj}x{nk}; float64 positions, uniform over the domain")
    stream = torch.cuda.current_stream().cuda_stream
    missed = 0
    for npoints in POINTS:
        pi = torch.rand(npoints, dtype=torch.float64, device="cuda", generator=gen) * (ni - 1)
        pj = torch.rand(npoints, dtype=torch.float64, device="cuda", generator=gen) * (nj - 1)
        pk = torch.rand(npoints, dtype=torch.float64, device="cuda", generator=gen) * (nk - 1)
        # today's route: indices into the whole arrays and weights, once, outside the timed region
        near_i, near_j = (torch.floor(p + 0.5).long() + HALO for p in (pi, pj))
        (i0, ti), (j0, tj), (k0, tk) = ((torch.floor(p).long(), (p - torch.floor(p)).to(tdt)) for p in (pi, pj, pk))
        i0, j0 = i0 + HALO, j0 + HALO
        i1, j1, k1 = (i0 + 1).clamp_(max=shape[0] - 1), (j0 + 1).clamp_(max=shape[1] - 1), (k0 + 1).clamp_(max=nk - 1)

        def torch_nearest(s, count):
            return [fields[s][n].tensor[near_i, near_j, :] for n in range(count)]

        def torch_linear(s, count):
            w0i, w1i, w0j, w1j = ((1 - ti)[:, None], ti[:, None], (1 - tj)[:, None], tj[:, None])
            out = []
            for n in range(count):
                t = fields[s][n].tensor
                out.append(w0j * (w0i * t[i0, j0, :] + w1i * t[i1, j0, :]) + w1j * (w0i * t[i0, j1, :] + w1i * t[i1, j1, :]))
            return out

        def torch_trilinear(s, count):
            out = []
            for n in range(count):
                t = fields[s][n].tensor
                planes = [(1 - tj) * ((1 - ti) * t[i0, j0, k] + ti * t[i1, j0, k]) + tj * ((1 - ti) * t[i0, j1, k] + ti * t[i1, j1, k]) for k in (k0, k1)]
                out.append((1 - tk) * planes[0] + tk * planes[1])
            return out

        routes = {("column", "nearest"): torch_nearest, ("column", "linear"): torch_linear, ("point", "linear"): torch_trilinear}
        # the same numbers?  A sanity check, not the contract: torch computes in the fields' dtype and orders the operations its own way
        tol = 1e-5 if dtype is np.float32 else 1e-13
        for (mode, method), route in routes.items():
            ours = sampling.sample(fields[0][0], pos_i=pi, pos_j=pj, pos_k=pk if mode == "point" else None, method=method, halo=HALO)[0]
            worst = float(np.abs(route(0, 1)[0].cpu().numpy().astype(np.float64) - ours).max())
            assert worst <= tol, f"torch indexing and the kernel disagree ({mode} {method}): {worst}"
        for count in (1, 8):
            for mode, method in ROWS:
                frozen = [sampling.Sample(fields[s][:count], pos_i=pi, pos_j=pj, pos_k=pk if mode == "point" else None, method=method, halo=HALO)
                          for s in range(SETS)]
                assert all(f.launches == 1 for f in frozen)
                t_k = event_us(lambda s: frozen[s](), calls)
                nbytes = frozen[0].result.nbytes
                padded = max(nbytes - nbytes % 16, 16)
                buf_in, buf_out = (torch.empty(padded, dtype=torch.uint8, device="cuda") for _ in range(2))
                t_b = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), padded, stream), calls)
                text = (f"  {npoints:>7} points, {count} field(s), {mode:<6} {method:<15} (k) {show(t_k)}   (b) copy of {nbytes / 2**20:7.2f} MiB "
                        f"{show(t_b)}, (k)/(b) = {t_k[1] / t_b[1]:.2f}")
                route = routes.get((mode, method))
                if route is None:
                    text += "; no (a): torch has no counterpart"
                else:
                    t_a = event_us(lambda s: route(s, count), calls)
                    disjoint = t_k[2] < t_a[0] or t_a[2] < t_k[0]
                    ok = t_k[1] <= t_a[1] and disjoint
                    missed |= 0 if ok else 1
                    text += f"; (a) {show(t_a)}, (k)/(a) = {t_k[1] / t_a[1]:.3f} (quartiles {'disjoint' if disjoint else 'overlap'}){'' if ok else '  MISSED'}"
                say(text)
                del frozen, buf_in, buf_out
    say(f"  {BAR} -> {'NOT met' if missed else 'met'}")
    return missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "point_sample_timing.txt"))
    ap.add_argument("--step", type=int, default=None, help="measure this shape alone, in this process (what the parent starts)")
    args = ap.parse_args()
    if args.step is not None:
        return measure(args.step, args.calls)
    lines = [f"HIP events around single calls, {WARMUP} warm-ups, {args.calls} timed calls, {SETS} sets of fields in rotation; "
             "median [first quartile, third quartile] in microseconds"]
    print(lines[0], flush=True)
    status = 0
    for step in range(len(SHAPES)):
        try:
            child = subprocess.run([sys.executable, __file__, "--step", str(step), "--calls", str(args.calls)], capture_output=True, text=True,
                                   timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            lines.append(f"\n{SHAPES[step][0]}: no result within {STEP_TIMEOUT} s; nothing further was started")
            status = 2
            break
        print(child.stdout + child.stderr[-2000:], flush=True)
        lines.append(child.stdout.rstrip("\n"))
        if child.returncode not in (0, 1):
            lines.append(f"\n{SHAPES[step][0]}: the measurement ended with status {child.returncode}; nothing further was started")
            status = 2
            break
        status = max(status, child.returncode)
    lines.append(f"\n{BAR}, both shapes -> {'met' if status == 0 else 'NOT met' if status == 1 else 'not decided'}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
