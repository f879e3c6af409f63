#!/usr/bin/env python3
"""per-call times of the Level-1 topology on the bench field (512^3, the bench's generator and isovalue): cx_level1_topology on a
fresh mesh (the edge table, the counts, the distinct vertices, the boundary loops and the records are one build: every post-pass makes
a new mesh, so it runs before each timed call, and so do the labels, which are not counted) and the cached calls of
cx_level1_topology and cx_level1_boundary_loops, next to cx_postprocess3d of the same mesh in the same process.  Warm context,
3 warm + `reps` timed calls between HIP events on the context's stream.  Prints one JSON line and writes it to
profiles/bench_topology_<size>.json."""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
dev = torch.device("cuda", 0)
A = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.adopt_device_grid(A.data_ptr(), tuple(A.shape), keepalive=A)
ctx.extract3d(0.0, 1)
post = ctx.postprocess3d(0)
nc, nl, nb = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
tab, lab, lp, vp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
counts = np.zeros(8, dtype=np.int64)


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


def fresh_mesh(k):
    ctx._check(ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data))
    ctx._check_attr(ctx.lib.cx_level1_component_labels(ctx.handle, ctypes.byref(lab), None))


def topology(k):
    return ctx.lib.cx_level1_topology(ctx.handle, ctypes.byref(nc), ctypes.byref(tab))


def loops(k):
    return ctx.lib.cx_level1_boundary_loops(ctx.handle, ctypes.byref(nl), ctypes.byref(nb), ctypes.byref(lp), ctypes.byref(vp))


live0 = _ffi.device_bytes(ctx.handle)[0]
out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "level1": post}
out["topology_fresh_mesh"] = timed(topology, before=fresh_mesh)
out["topology_device_bytes"] = _ffi.device_bytes(ctx.handle)[0] - live0
out["topology_cached"] = timed(topology)
out["boundary_loops_cached"] = timed(loops)
out["postprocess3d"] = timed(lambda k: ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data))
table = ctx.level1_topology()
L, V = ctx.level1_boundary_loops()
big = int(np.argmax(table["triangles"]))
out.update(components=len(table), loops=len(L), boundary_edges=len(V), longest_loop=int(L["count"].max()) if len(L) else 0,
           nonsimple_loops=int(table["nonsimple_loops"].sum()), nonmanifold_edges=int(table["nonmanifold_edges"].sum()),
           edges=int(table["edges"].sum()), edge_table_bytes=(4 * int(post["n_triangles"]) + 64) * 16,
           largest={k: int(table[k][big]) for k in table.dtype.names})
ctx.close()
line = json.dumps(out)
print(line)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_topology_%d.json" % size), "w") as f:
    f.write(line + "\n")
