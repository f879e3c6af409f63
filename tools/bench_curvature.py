#!/usr/bin/env python3
"""per-call times of the vertex curvature on the bench field (512^3, the bench's generator and isovalue): cx_level0_curvature and
cx_level1_curvature next to cx_level0_normals (the yardstick: 12 requested samples per vertex against 38), cx_level1_normals and the
vertex stage of the same extraction in the same process (cx_timing_read).  Warm context, several calls, HIP events on the context's
stream; prints one JSON line and writes it to profiles/bench_curvature_<N>.json."""
import ctypes, json, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
A = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.adopt_device_grid(A.data_ptr(), tuple(A.shape), keepalive=A)
for _ in range(3):
    c = ctx.extract3d(0.0, 1)
ctx.timing_enable(True)
for _ in range(reps):
    c = ctx.extract3d(0.0, 1)
T = ctx.timing_read()
ctx.timing_enable(False)
vertex_stage_ms = T["cells_ms"] / max(1, T["n"])
post = ctx.postprocess3d(0)
out = ctypes.c_void_p()


def timed(call):
    "median / min / max milliseconds of `reps` calls after 3 warm ones, each between two events on the context's stream"
    for _ in range(3):
        ctx._check_attr(call())
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx._check_attr(call())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


n0 = timed(lambda: ctx.lib.cx_level0_normals(ctx.handle, None, ctypes.byref(out)))
c0 = timed(lambda: ctx.lib.cx_level0_curvature(ctx.handle, None, ctypes.byref(out)))
n1 = timed(lambda: ctx.lib.cx_level1_normals(ctx.handle, None, ctypes.byref(out)))
c1 = timed(lambda: ctx.lib.cx_level1_curvature(ctx.handle, None, ctypes.byref(out)))
nv, nv1 = int(c["n_vertices"]), int(post["n_vertices"])
line = json.dumps({"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "level0": c, "level1_vertices": nv1,
                   "vertex_stage_ms": round(vertex_stage_ms, 4), "level0_normals": n0, "level0_curvature": c0, "level1_normals": n1,
                   "level1_curvature": c1,
                   "level0_curvature_over_normals": round(c0["median_ms"] / n0["median_ms"], 2),
                   "requested_samples_ratio": round(38 / 12, 2),
                   "level1_curvature_over_normals": round(c1["median_ms"] / n1["median_ms"], 2),
                   "level0_curvature_over_vertex_stage": round(c0["median_ms"] / vertex_stage_ms, 2) if vertex_stage_ms else None,
                   "level0_normals_Mvertices_per_s": round(nv / n0["median_ms"] / 1e3, 1),
                   "level0_curvature_Mvertices_per_s": round(nv / c0["median_ms"] / 1e3, 1),
                   "level1_curvature_Mvertices_per_s": round(nv1 / c1["median_ms"] / 1e3, 1)})
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
open(os.path.join(ROOT, "profiles", "bench_curvature_%d.json" % size), "w").write(line + "\n")
