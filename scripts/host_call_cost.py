import sys, time
import os; R=os.path.join(os.path.dirname(os.path.abspath(__file__)),'..'); sys.path.insert(0,R); sys.path.insert(0,os.path.join(R,'tests'))
import numpy as np, torch
import gt4py_amd.storage as gt_storage
from gt4py_amd.cartesian import gtscript
import stencil_zoo as zoo
for name in ("laplacian","vertical_advection_dycore","horizontal_diffusion","two_stage_written_input","cross_column_recurrence"):
    defn, ext, scal, opts = zoo.ZOO[name]
    for use_lib in ((True, False) if name in ("laplacian", "horizontal_diffusion") else (False,)):
        obj = gtscript.stencil(backend="hip:mi300", definition=defn, externals=ext, device_sync=False, use_kernel_library=use_lib)
        domain=(16,16,8)
        arrays, origins = zoo.make_inputs(obj, domain)
        dev = {k: gt_storage.from_array(v, dtype=v.dtype, backend="hip:mi300", aligned_index=origins[k]) for k,v in arrays.items()}
        frozen = obj.freeze(origin=origins, domain=domain)
        for _ in range(20): frozen(**dev, **scal)
        torch.cuda.synchronize()
        t=time.perf_counter(); n=2000
        for _ in range(n): frozen(**dev, **scal)
        t1=time.perf_counter(); torch.cuda.synchronize()
        print(f"{name:28s} {'library' if use_lib else 'generated':9s} frozen call host cost {(t1-t)/n*1e6:6.1f} us")
        t=time.perf_counter()
        for _ in range(n): obj(**dev, **scal, origin=origins, domain=domain)
        t1=time.perf_counter(); torch.cuda.synchronize()
        print(f"{name:28s} {'library' if use_lib else 'generated':9s} full   call host cost {(t1-t)/n*1e6:6.1f} us")

# launch-bound loop: 20 dependent small applies, eager vs one hipGraph replay
defn, ext, scal, opts = zoo.ZOO["laplacian"]
obj = gtscript.stencil(backend="hip:mi300", definition=defn, device_sync=False)
domain = (128, 128, 64)
shape = (130, 130, 64)
a = gt_storage.ones(shape, backend="hip:mi300", aligned_index=(1, 1, 0))
b = gt_storage.ones(shape, backend="hip:mi300", aligned_index=(1, 1, 0))
fr = obj.freeze(origin={"inp": (1, 1, 0), "out": (1, 1, 0)}, domain=domain)


def loop():
    for _ in range(10):
        fr(inp=a, out=b)
        fr(inp=b, out=a)


loop(); torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(50): loop()
torch.cuda.synchronize()
eager = (time.perf_counter() - t) / 50
g = torch.cuda.CUDAGraph()
with torch.cuda.graph(g):
    loop()
g.replay(); torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(50): g.replay()
torch.cuda.synchronize()
graph = (time.perf_counter() - t) / 50
print(f"20 dependent 128x128x64 Laplacian applies: eager {eager*1e6:7.1f} us, hipGraph replay {graph*1e6:7.1f} us")

# frozen utility calls (boundary, diagnostics, transfer, vertical, horizontal): host cost of one call, 16 x 16 x 8 domain, halo 2.
# Five repeats of 2 000 calls with one synchronisation at the end of each; the median and the spread (max - min) of the five.
import statistics
from gt4py_amd import boundary, diagnostics, horizontal, transfer, vertical


def _frozen_utilities():
    def field(nk=8):
        return gt_storage.zeros((20, 20, nk), backend="hip:mi300", aligned_index=(2, 2, 0))

    a, b, c, d, pi, pj = (field() for _ in range(6))  # (named: a frozen call holds weak references to what it was given)
    zs = gt_storage.from_array(np.arange(9.0), backend="hip:mi300")
    zd = gt_storage.from_array(np.arange(9.0), backend="hip:mi300")
    yield "HaloFill", boundary.HaloFill([a, b], halo=2, mode="periodic")
    yield "FieldStats", diagnostics.FieldStats([a, b], halo=2)
    yield "LevelStats", diagnostics.LevelStats([a, b], halo=2)
    yield "FieldCopy", transfer.FieldCopy([c, d], [a, b], halo=2)
    yield "VerticalRemap", vertical.VerticalRemap([c, d], [a, b], src_edges=zs, dst_edges=zd, method="plm", halo=2)
    yield "HorizontalInterp", horizontal.HorizontalInterp([c, d], [a, b], pos_i=pi, pos_j=pj, relative=True, method="cubic", halo=2)


print(f"{'frozen utility call':18s} {'median us':>10s} {'spread us':>10s}   five repeats of 2000 calls (us per call)")
for name, call in _frozen_utilities():
    assert tuple(getattr(call, "domain", (16, 16, 8)))[:2] == (16, 16)
    for _ in range(20): call()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(2000): call()
        t1 = time.perf_counter(); torch.cuda.synchronize()
        per_call.append((t1 - t) / 2000 * 1e6)
    print(f"{name:18s} {statistics.median(per_call):10.2f} {max(per_call) - min(per_call):10.2f}   " + " ".join(f"{x:6.2f}" for x in per_call))
