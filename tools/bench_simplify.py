#!/usr/bin/env python3
"""per-call times of the simplification of the Level-1 mesh on the bench field (512^3, the bench's generator and isovalue): cells 2, 4
and 8 with and without carried normals, the dry run, and a `target_triangles` search for 1 M triangles, next to cx_postprocess3d and
cx_level1_normals of the same mesh in the same process.  Warm context, 3 warm + `reps` timed calls between HIP events on the
context's stream.  A simplification consumes its input, so every timed call is preceded by an untimed cx_postprocess3d (and, with
normals, cx_level1_normals and the component labels, which the call would otherwise make itself: they are timed on their own).
Prints one JSON line and writes it to profiles/bench_simplify_<size>.json."""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
A = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.adopt_device_grid(A.data_ptr(), tuple(A.shape), keepalive=A)
ctx.extract3d(0.0, 1)
post = ctx.postprocess3d(0)
counts, sc, q = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64), ctypes.c_double(0.0)
lab, nrm = ctypes.c_void_p(), ctypes.c_void_p()


def timed(call, n=reps, before=None):
    "median / min / max milliseconds of n calls after 3 warm ones, each between two events on the context's stream"
    ms = []
    for k in range(3 + n):
        if before:
            before(k)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx._check_attr(call(k))
        e1.record()
        e1.synchronize()
        if k >= 3:
            ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def restore(normals):
    "the full mesh again, with everything a simplification reads but does not own already made"
    def go(k):
        ctx._check(ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data))
        ctx._check_attr(ctx.lib.cx_level1_component_labels(ctx.handle, None, ctypes.byref(lab)))
        if normals:
            ctx._check_attr(ctx.lib.cx_level1_normals(ctx.handle, None, ctypes.byref(nrm)))
    return go


def simplify(cell, flags):
    c3 = np.array([cell, cell, cell], dtype=np.float64)
    return lambda k: ctx.lib.cx_level1_simplify(ctx.handle, c3.ctypes.data, flags, sc.ctypes.data, ctypes.byref(q))


few = max(3, reps // 4)
out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "level1": post}
for cell in (2.0, 4.0, 8.0):
    for normals in (False, True):
        name = "cell_%g%s" % (cell, "_normals" if normals else "")
        out[name] = timed(simplify(cell, _ffi.CX_SIMPLIFY_NORMALS if normals else 0), n=few, before=restore(normals))
        out[name].update(vertices=int(sc[0]), triangles=int(sc[1]), clusters=int(sc[6]), distinct=int(sc[7]))
restore(False)(0)
out["dry_run_cell_4"] = timed(simplify(4.0, _ffi.CX_SIMPLIFY_COUNT_ONLY))
out["postprocess3d"] = timed(lambda k: ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data), n=few)
out["normals"] = timed(lambda k: ctx.lib.cx_level1_normals(ctx.handle, None, ctypes.byref(nrm)))
out["labels"] = timed(lambda k: ctx.lib.cx_level1_component_labels(ctx.handle, None, ctypes.byref(lab)), n=few,
                      before=lambda k: ctx._check(ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data)))


# target_triangles = 1 M through the Python layer's search (dry runs, then one simplification), on the context above
class _Owner(object):
    pass


from contourist_amd import tetrahedral
owner, target = _Owner(), 1000000
found = {}


def search(k):
    found.update(tetrahedral._simplify_on(ctx, None, target, True, True, False, size - 1, owner))
    return 0


out["target_triangles_1M"] = timed(search, n=few, before=restore(False))
out["target_triangles_1M"].update(cell=found["cell"][0], triangles=found["n_triangles"], dry_runs=len(owner._simplify_search))
out["cell_4_over_postprocess3d"] = round(out["cell_4"]["median_ms"] / out["postprocess3d"]["median_ms"], 3)
ctx.close()
line = json.dumps(out)
print(line)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_simplify_%d.json" % size), "w") as f:
    f.write(line + "\n")
