"""Host cost of one ``__call__`` of each of the nine frozen utility calls, in the manner of host_call_cost.py: two fields, 16 x 16 x 8
domain, halo 2; per class 20 warm-up calls, then five repeats of 2 000 calls, ``perf_counter`` around the loop with one
synchronisation after it.  Prints the median and the five repeats (us per call).

    python scripts/utility_call_cost.py [TREE]      # TREE: the checkout whose gt4py_amd is measured, default this one
"""
import os
import statistics
import sys
import time

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gt4py_amd.storage as gt_storage
from gt4py_amd import boundary, diagnostics, horizontal, linesolve, transfer, vertical

assert os.path.abspath(boundary.__file__).startswith(ROOT), boundary.__file__


def frozen_utilities():
    def field(fill=0.0):
        return gt_storage.from_array(np.full((20, 20, 8), fill), backend="hip:mi300", aligned_index=(2, 2, 0))

    a, b, c, d, pi, pj = (field() for _ in range(6))  # (named: a frozen call holds weak references to what it was given)
    lower, diag, upper = field(-1.0), field(4.0), field(-1.0)
    edges_s = gt_storage.from_array(np.arange(9.0), backend="hip:mi300")
    edges_d = gt_storage.from_array(np.arange(9.0), backend="hip:mi300")
    levels_s = gt_storage.from_array(np.arange(8.0), backend="hip:mi300")
    levels_d = gt_storage.from_array(np.arange(8.0) + 0.5, backend="hip:mi300")
    coarse = [gt_storage.zeros((8, 8, 8), backend="hip:mi300") for _ in range(2)]
    x = np.arange(17.0)
    yield "HaloFill", boundary.HaloFill([a, b], halo=2, mode="periodic")
    yield "FieldStats", diagnostics.FieldStats([a, b], halo=2)
    yield "LevelStats", diagnostics.LevelStats([a, b], halo=2)
    yield "FieldCopy", transfer.FieldCopy([c, d], [a, b], halo=2)
    yield "VerticalRemap", vertical.VerticalRemap([c, d], [a, b], src_edges=edges_s, dst_edges=edges_d, method="plm", halo=2)
    yield "VerticalInterp", vertical.VerticalInterp([c, d], [a, b], src_coord=levels_s, dst_coord=levels_d, method="cubic", halo=2)
    yield "HorizontalInterp", horizontal.HorizontalInterp([c, d], [a, b], pos_i=pi, pos_j=pj, relative=True, method="cubic", halo=2)
    yield "HorizontalRemap", horizontal.HorizontalRemap(coarse, [a, b], src_edges=(x, x), dst_edges=(x[::2], x[::2]), method="plm",
                                                        src_origin=(2, 2, 0))
    yield "LineSolve", linesolve.LineSolve([c, d], [a, b], lower=lower, diag=diag, upper=upper, axis="I", halo=2)


print(f"tree {ROOT}")
print(f"{'frozen utility call':18s} {'median us':>10s}   five repeats of 2000 calls (us per call)")
for name, call in frozen_utilities():
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(2000):
            call()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        per_call.append((t1 - t) / 2000 * 1e6)
    print(f"{name:18s} {statistics.median(per_call):10.2f}   " + " ".join(f"{v:6.2f}" for v in per_call), flush=True)
