"""What a 3-d departure-point interpolation costs (output kept as profiles/departure_interp_timing.txt).

Per shape, number of fields (1 and 8) and method, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3
sets of fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.departure.DepartureInterp call of all the fields (frozen form: one launch per 8 fields), displacements of a
      smooth 3-d flow -- a solid-body rotation about the centre of the domain in I and J and a standing wave along K, at most 2
      cells per axis -- in three IJK position fields of the fields' dtype, relative mode;
  (a) torch.nn.functional.grid_sample on the 5-d view (1, 1, nk, nj, ni) of the same tensors (mode "bilinear" = trilinear,
      align_corners=True, padding_mode="border"), the grid built once outside the timed region, one call per field, the result
      copied into the destination's box: for `linear` only (torch has no tricubic);
  (b) the split pair horizontal.HorizontalInterp + vertical.VerticalInterp on the same displacements, which computes LESS: the
      vertical step reads the column at (i, j), not the one at the horizontal departure position;
  (c) gt4mi_stream_copy of the algorithmic bytes: src + dst per field, plus the three position fields once.

Bar: `linear` with 8 fields, (k) <= (a) by medians with disjoint quartile ranges, for both shapes.  The script exits non-zero
when the bar is missed.  (k)/(b) and (k)/(c) are recorded and carry no bar.

Every shape is measured in a child process of its own under a time limit; the parent opens no device, stops at the first child
that fails and writes what was measured so far.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/departure_interp_timing.py --step 0, in a run of its own.
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
METHODS = ("linear", "cubic", "cubic_monotone")
BAR = "bar: linear, 8 fields: (k) <= (a) by medians with disjoint quartiles"


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


def measure(step: int, calls: int) -> int:
    """One shape, in this process; prints the lines of the profile.  Returns 1 when the bar is missed."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import _lib, departure, horizontal, vertical

    say = lambda text="": print(text, flush=True)  # noqa: E731
    backend = "hip:mi300"
    lib = _lib.load()
    name, shape, dtype = SHAPES[step]
    tdt = torch.float32 if dtype is np.float32 else torch.float64
    itemsize = np.dtype(dtype).itemsize
    gen = torch.Generator(device="cuda").manual_seed(1)
    ni, nj, nk = shape[0] - 2 * HALO, shape[1] - 2 * HALO, shape[2]
    origin = (HALO, HALO, 0)
    box = (slice(HALO, HALO + ni), slice(HALO, HALO + nj))

    def storage(values=None):
        s = gt_storage.zeros(shape, dtype, backend=backend, aligned_index=origin)
        if values is not None:
            s.tensor.copy_(values)
        return s

    # the smooth flow: solid-body rotation about the centre in I and J (the largest displacement 2, at the corners), a standing wave
    # of amplitude 2 along K
    ci, cj = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    omega = 2.0 / float(np.hypot(ci, cj))
    gi = torch.arange(shape[0], dtype=torch.float64, device="cuda").reshape(-1, 1, 1)
    gj = torch.arange(shape[1], dtype=torch.float64, device="cuda").reshape(1, -1, 1)
    gk = torch.arange(shape[2], dtype=torch.float64, device="cuda").reshape(1, 1, -1)
    one = torch.ones(shape, dtype=torch.float64, device="cuda")
    di = storage((omega * (gj - cj) * one).to(tdt))
    dj = storage((-omega * (gi - ci) * one).to(tdt))
    dk = storage((2.0 * torch.sin(2 * np.pi * gi / shape[0]) * torch.cos(2 * np.pi * gj / shape[1]) * torch.sin(np.pi * gk / max(nk - 1, 1))).to(tdt))
    del one
    srcs = [[storage(torch.rand(shape, dtype=tdt, device="cuda", generator=gen)) for _ in range(8)] for _ in range(SETS)]
    dsts = [[storage() for _ in range(8)] for _ in range(SETS)]
    tmps = [storage() for _ in range(8)]  # what the split pair hands from its horizontal to its vertical step
    # the split pair's coordinates: the levels themselves (a Field[K]) and the departure levels k + dk
    # (the vertical step works on views of the compute domain: it has no reach, and the objects hold weak references to the views)
    levels = torch.arange(nk, dtype=tdt, device="cuda")
    depart_k = storage((gk + dk.tensor.to(torch.float64)).to(tdt)).tensor[box]
    tmp_views = [t.tensor[box] for t in tmps]
    dst_views = [[d.tensor[box] for d in dsts[s]] for s in range(SETS)]
    # grid_sample: the field as (1, 1, D = nk, H = nj, W = ni) -- a permuted view --, the grid (1, nk, nj, ni, 3) in [-1, 1] over the
    # WHOLE array, x -> W (I), y -> H (J), z -> D (K); positions clamped as the kernel clamps them
    x = (gi[box[0]] + di.tensor[box].to(torch.float64)).clamp_(0, shape[0] - 1) * (2.0 / (shape[0] - 1)) - 1.0
    y = (gj[:, box[1]] + dj.tensor[box].to(torch.float64)).clamp_(0, shape[1] - 1) * (2.0 / (shape[1] - 1)) - 1.0
    z = (gk + dk.tensor[box].to(torch.float64)).clamp_(0, nk - 1) * (2.0 / max(nk - 1, 1)) - 1.0
    grid = torch.stack([x.permute(2, 1, 0), y.permute(2, 1, 0), z.permute(2, 1, 0)], dim=-1).unsqueeze(0).to(tdt).contiguous()
    del x, y, z

    def grid_route(s, count):
        for n in range(count):
            out = torch.nn.functional.grid_sample(srcs[s][n].tensor.permute(2, 1, 0)[None, None], grid, mode="bilinear", padding_mode="border",
                                                  align_corners=True)
            dsts[s][n].tensor[box].copy_(out[0, 0].permute(2, 1, 0))

    # the same numbers?  A sanity check, not the contract: torch computes in the fields' dtype and orders the operations its own way
    tol = 5e-3 if dtype is np.float32 else 1e-9
    grid_route(0, 1)
    departure.interpolate_3d(dsts[0][1], srcs[0][0], pos_i=di, pos_j=dj, pos_k=dk, method="linear", relative=True, halo=HALO)
    torch.cuda.synchronize()
    worst = float((dsts[0][0].tensor[box] - dsts[0][1].tensor[box]).abs().max())
    assert worst <= tol, f"grid_sample and the kernel disagree: {worst}"
    say(f"\n{name} arrays, halo {HALO}, domain {ni}x{nj}x{nk}; positions: three IJK fields of the fields' dtype")
    stream = torch.cuda.current_stream().cuda_stream
    missed = 0
    for count in (1, 8):
        algorithmic = (2 * count + 3) * ni * nj * nk * itemsize
        half = algorithmic // 2 - (algorithmic // 2) % 16
        buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
        t_c = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), calls)
        say(f"  {count} field(s): (c) gt4mi_stream_copy, {algorithmic / 2**20:6.0f} MiB in + out            {show(t_c)}")
        del buf_in, buf_out
        t_a = event_us(lambda s: grid_route(s, count), calls)
        say(f"  {count} field(s): (a) grid_sample trilinear, one call per field      {show(t_a)}")
        for method in METHODS:
            frozen = [departure.DepartureInterp(dsts[s][:count], srcs[s][:count], pos_i=di, pos_j=dj, pos_k=dk, method=method, relative=True,
                                                halo=HALO) for s in range(SETS)]
            assert all(f.launches == 1 for f in frozen)
            t_k = event_us(lambda s: frozen[s](), calls)
            split = [(horizontal.HorizontalInterp(tmps[:count], srcs[s][:count], pos_i=di, pos_j=dj, method=method, relative=True, halo=HALO),
                      vertical.VerticalInterp(dst_views[s][:count], tmp_views[:count], src_coord=levels, dst_coord=depart_k, method=method))
                     for s in range(SETS)]

            def split_route(s):
                split[s][0]()
                split[s][1]()

            t_b = event_us(split_route, calls)
            text = (f"  {count} field(s): (k) DepartureInterp {method:<15} {show(t_k)}   {algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; "
                    f"(b) split pair {show(t_b)}, (k)/(b) = {t_k[1] / t_b[1]:.2f}; (k)/(c) = {t_k[1] / t_c[1]:.2f}")
            if method == "linear":
                disjoint = t_k[2] < t_a[0] or t_a[2] < t_k[0]
                text += f"; (k)/(a) = {t_k[1] / t_a[1]:.3f} (quartiles {'disjoint' if disjoint else 'overlap'})"
                if count == 8 and not (t_k[1] <= t_a[1] and disjoint):
                    missed = 1
            say(text)
    say(f"  {BAR} -> {'NOT met' if missed else 'met'}")
    return missed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "departure_interp_timing.txt"))
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
