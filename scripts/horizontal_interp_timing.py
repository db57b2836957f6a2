"""What a horizontal interpolation at run-time positions costs (output kept as profiles/horizontal_interp_timing.txt).

Per shape, number of fields (1 and 8) and method, side by side (HIP events around single calls, 5 warm-ups, 30 timed calls, 3
sets of fields in rotation so that the 256 MiB Infinity Cache does not serve repeats; median and quartiles):
  (k) one gt4py_amd.horizontal.HorizontalInterp call of all the fields (frozen form: one launch per 8 fields), displacements of a
      smooth flow -- a solid-body rotation about the centre of the domain, |displacement| <= 2 -- in a Field[IJ], relative mode;
  (a) the torch routes a user has without it, on the same tensors:
      (a1) floor / clamp / advanced-indexing gathers / lerp (linear) or weighted sums of the 16 gathers (cubic, the same Lagrange
           weights); the indices and weights are computed once per call, the gathers run once per field;
      (a2) torch.nn.functional.grid_sample(align_corners=True, padding_mode="border"), mode "bilinear" for linear and "bicubic"
           for the cubics (a cubic convolution, not the Lagrange cubic: the cost of the route, not the same numbers), on a
           permuted view of the same tensors, once per field;
  (b) gt4mi_stream_copy of the algorithmic bytes: src + dst per field, plus the two position fields once;
  (c) the same call as (k) with uniformly random absolute positions across the domain (every lane reads lines of its own).

Bar: (k) <= (a1) and (k) <= (a2) by medians for the same fields on the smooth flow, no margin; the output also says whether the
quartile ranges are disjoint.  The script exits non-zero when the bar is missed.  (k)/(b) and (c) are reported and carry no bar.

Kernel time alone: rocprofv3 --kernel-trace --stats -- python scripts/horizontal_interp_timing.py, in a run of its own.
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
HALO = 3
SHAPES = (("1024x1024x80 float32", (1024, 1024, 80), np.float32),
          ("512x512x128 float64", (512, 512, 128), np.float64))
METHODS = ("linear", "cubic", "cubic_monotone")


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


def taps(x, lo, hi, cubic):
    """Indices (into the array: + HALO) and weights of one axis from clamped positions x, as torch tensors."""
    import torch

    x0 = torch.floor(x)
    t = x - x0
    b = x0.to(torch.int64)
    if not cubic:
        return [(b + m).clamp_(lo, hi) + HALO for m in (0, 1)], [t]
    a, c, d = t + 1.0, t - 1.0, t - 2.0
    w = [-(t * c * d) / 6.0, (a * c * d) / 2.0, -(a * t * d) / 2.0, (a * t * c) / 6.0]
    return [(b + m).clamp_(lo, hi) + HALO for m in (-1, 0, 1, 2)], w


def torch_route(dsts, srcs, di, dj, index_i, index_j, domain, cubic):
    """(a1): the indices and weights once, then per field the gathers and their combination."""
    import torch

    ni, nj, _ = domain
    x = (index_i + di).clamp_(-HALO, ni - 1 + HALO)
    y = (index_j + dj).clamp_(-HALO, nj - 1 + HALO)
    ii, wi = taps(x, -HALO, ni - 1 + HALO, cubic)
    jj, wj = taps(y, -HALO, nj - 1 + HALO, cubic)
    wi, wj = [w.unsqueeze(-1) for w in wi], [w.unsqueeze(-1) for w in wj]
    for dst, src in zip(dsts, srcs):
        if cubic:
            out = None
            for r in range(4):
                row = wi[0] * src[ii[0], jj[r]]
                for c in range(1, 4):
                    row = row + wi[c] * src[ii[c], jj[r]]
                out = wj[r] * row if out is None else out + wj[r] * row
        else:
            r0 = torch.lerp(src[ii[0], jj[0]], src[ii[1], jj[0]], wi[0])
            r1 = torch.lerp(src[ii[0], jj[1]], src[ii[1], jj[1]], wi[0])
            out = torch.lerp(r0, r1, wj[0])
        dst[HALO:HALO + ni, HALO:HALO + nj].copy_(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "horizontal_interp_timing.txt"))
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
    for name, shape, dtype in SHAPES:
        tdt = torch.float32 if dtype is np.float32 else torch.float64
        itemsize = np.dtype(dtype).itemsize
        gen = torch.Generator(device="cuda").manual_seed(1)
        ni, nj, nk = shape[0] - 2 * HALO, shape[1] - 2 * HALO, shape[2]
        domain = (ni, nj, nk)
        origin = (HALO, HALO, 0)

        def storage(full_shape, values=None):
            s = gt_storage.zeros(full_shape, dtype, backend=backend, aligned_index=origin[:len(full_shape)], dimensions=list("IJK")[:len(full_shape)])
            if values is not None:
                s.tensor.copy_(values)
            return s

        # the smooth flow: solid-body rotation about the centre, the largest displacement 2 (at the corners)
        ci, cj = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
        omega = 2.0 / float(np.hypot(ci, cj))
        gi = torch.arange(shape[0], dtype=torch.float64, device="cuda").unsqueeze(1).expand(shape[0], shape[1])
        gj = torch.arange(shape[1], dtype=torch.float64, device="cuda").unsqueeze(0).expand(shape[0], shape[1])
        di = storage(shape[:2], (omega * (gj - cj)).to(tdt))
        dj = storage(shape[:2], (-omega * (gi - ci)).to(tdt))
        # the scattered positions: absolute, uniform across the domain
        ri = storage(shape[:2], torch.rand(shape[:2], dtype=torch.float64, device="cuda", generator=gen).mul_(ni - 1).to(tdt))
        rj = storage(shape[:2], torch.rand(shape[:2], dtype=torch.float64, device="cuda", generator=gen).mul_(nj - 1).to(tdt))
        srcs = [[storage(shape, torch.rand(shape, dtype=tdt, device="cuda", generator=gen)) for _ in range(8)] for _ in range(SETS)]
        dsts = [[storage(shape) for _ in range(8)] for _ in range(SETS)]
        check = storage(shape)
        box = (slice(HALO, HALO + ni), slice(HALO, HALO + nj))
        d_i, d_j = di.tensor[box], dj.tensor[box]
        index_i = torch.arange(ni, dtype=tdt, device="cuda").unsqueeze(1).expand(ni, nj)
        index_j = torch.arange(nj, dtype=tdt, device="cuda").unsqueeze(0).expand(ni, nj)
        # grid_sample: the field as (1, C = nk, H = nj, W = ni) -- a permuted view --, the grid (1, nj, ni, 2) in [-1, 1] over the WHOLE array
        grid = torch.stack([((index_i + d_i + HALO) * (2.0 / (shape[0] - 1)) - 1.0).t(), ((index_j + d_j + HALO) * (2.0 / (shape[1] - 1)) - 1.0).t()],
                           dim=-1).unsqueeze(0).contiguous()

        def grid_route(s, count, mode):
            for n in range(count):
                out = torch.nn.functional.grid_sample(srcs[s][n].tensor.permute(2, 1, 0).unsqueeze(0), grid, mode=mode, padding_mode="border",
                                                      align_corners=True)
                dsts[s][n].tensor[box].copy_(out[0].permute(2, 1, 0))

        # the same numbers?  A sanity check, not the contract: torch computes the positions in the fields' dtype (the kernel in
        # float64) and orders the operations its own way, so float32 positions on 1024 points differ by ~1e-4 of a cell
        tol = 5e-3 if dtype is np.float32 else 1e-9
        for method in ("linear", "cubic"):
            torch_route([check.tensor], [srcs[0][0].tensor], d_i, d_j, index_i, index_j, domain, method == "cubic")
            horizontal.interpolate(dsts[0][0], srcs[0][0], pos_i=di, pos_j=dj, method=method, relative=True, halo=HALO)
            torch.cuda.synchronize()
            worst = float((dsts[0][0].tensor[box] - check.tensor[box]).abs().max())
            assert worst <= tol, f"the torch route and the kernel disagree ({method}): {worst}"
        grid_route(0, 1, "bilinear")
        horizontal.interpolate(dsts[0][1], srcs[0][0], pos_i=di, pos_j=dj, method="linear", relative=True, halo=HALO)
        torch.cuda.synchronize()
        worst = float((dsts[0][0].tensor[box] - dsts[0][1].tensor[box]).abs().max())
        assert worst <= tol, f"grid_sample and the kernel disagree: {worst}"
        say(f"\n{name} arrays, halo {HALO}, domain {ni}x{nj}x{nk}; positions: Field[IJ] of the fields' dtype")
        stream = torch.cuda.current_stream().cuda_stream
        for count in (1, 8):
            algorithmic = 2 * count * ni * nj * nk * itemsize + 2 * ni * nj * itemsize
            half = algorithmic // 2 - (algorithmic // 2) % 16
            buf_in, buf_out = (torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(2))
            t_b = event_us(lambda s: lib.gt4mi_stream_copy(buf_in.data_ptr(), buf_out.data_ptr(), half, stream), args.calls)
            say(f"  {count} field(s): (b) gt4mi_stream_copy, {algorithmic / 2**20:6.0f} MiB in + out      {show(t_b)}")
            del buf_in, buf_out
            baselines = {}
            for cubic in (False, True):
                label = "cubic" if cubic else "linear"
                baselines[label] = [
                    (f"(a1) torch gathers, {label}", event_us(lambda s: torch_route([d.tensor for d in dsts[s][:count]], [x.tensor for x in srcs[s][:count]],
                                                                                     d_i, d_j, index_i, index_j, domain, cubic), args.calls)),
                    (f"(a2) grid_sample {'bicubic' if cubic else 'bilinear'}", event_us(lambda s: grid_route(s, count, "bicubic" if cubic else "bilinear"),
                                                                                       args.calls))]
                for what, t in baselines[label]:
                    say(f"  {count} field(s): {what:<42} {show(t)}")
            for method in METHODS:
                frozen = [horizontal.HorizontalInterp(dsts[s][:count], srcs[s][:count], pos_i=di, pos_j=dj, method=method, relative=True, halo=HALO)
                          for s in range(SETS)]
                assert all(f.launches == 1 for f in frozen)
                t_k = event_us(lambda s: frozen[s](), args.calls)
                against = baselines["linear" if method == "linear" else "cubic"]
                ratios = ", ".join(f"(k)/{what[:4]} = {t_k[1] / t[1]:.3f} (quartiles {'disjoint' if t_k[2] < t[0] or t[2] < t_k[0] else 'overlap'})"
                                   for what, t in against)
                say(f"  {count} field(s): (k) HorizontalInterp {method:<15} smooth   {show(t_k)}   "
                    f"{algorithmic / (t_k[1] * 1e-6) / 1e12:.2f} TB/s algorithmic; {ratios}, (k)/(b) = {t_k[1] / t_b[1]:.2f}")
                for what, t in against:
                    if t_k[1] > t[1]:
                        missed.append(f"{name} {count} field(s) {method}: (k) {t_k[1]:.1f} > {what[:4]} {t[1]:.1f}")
                scattered = [horizontal.HorizontalInterp(dsts[s][:count], srcs[s][:count], pos_i=ri, pos_j=rj, method=method, halo=HALO)
                             for s in range(SETS)]
                t_c = event_us(lambda s: scattered[s](), args.calls)
                say(f"  {count} field(s): (c) HorizontalInterp {method:<15} scattered {show(t_c)}   (c)/(k) = {t_c[1] / t_k[1]:.2f}")
        del srcs, dsts, check, di, dj, ri, rj, grid
        torch.cuda.empty_cache()
    say(f"\nbar: (k) <= (a1) and (k) <= (a2) by medians for the same fields on the smooth flow -> "
        f"{'met' if not missed else 'NOT met: ' + '; '.join(missed)}")
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
    return 0 if not missed else 1


if __name__ == "__main__":
    sys.exit(main())
