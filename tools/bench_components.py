#!/usr/bin/env python3
"""per-call times of the Level-1 components on the bench field (512^3, the bench's generator and isovalue): labels, measures (first
call and cached) and `keep largest 1`, next to cx_postprocess3d and cx_level1_normals of the same mesh in the same process.  Warm
context, 3 warm + `reps` timed calls between HIP events on the context's stream.  The measure kernel reads 12 + 72 bytes per
triangle: the rate of the whole call (accumulator reset, measure kernel, vertex count, finish: the measure kernel is all but a few
microseconds of it) is printed next to the streaming-read figure of cx_measure_read_bandwidth on the same device.
Prints one JSON line and writes it to profiles/bench_components_<size>.json."""
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
nc, tab, lab = ctypes.c_int64(0), ctypes.c_void_p(), ctypes.c_void_p()
md = [np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0 + 2.0 ** -20 * k]) for k in range(2)]     # two mappings: alternating them defeats the cache


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


def measures(k):
    return ctx.lib.cx_level1_components(ctx.handle, md[k & 1].ctypes.data, ctypes.byref(nc), ctypes.byref(tab), None)


ctx._check_attr(ctx.lib.cx_level1_component_labels(ctx.handle, ctypes.byref(lab), None))
nt, nv = int(post["n_triangles"]), int(post["n_vertices"])
first = timed(measures)
out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "level1": post, "measures_first_call": first,
       "measure_bytes_per_triangle": 84, "measures_call_GB_per_s": round(nt * 84 / first["median_ms"] / 1e6, 1)}
out["measures_cached"] = timed(lambda k: ctx.lib.cx_level1_components(ctx.handle, md[0].ctypes.data, ctypes.byref(nc), ctypes.byref(tab), None))
out["components"] = int(nc.value)
out["normals"] = timed(lambda k: ctx.lib.cx_level1_normals(ctx.handle, None, ctypes.byref(tab)))
counts = np.zeros(8, dtype=np.int64)
out["postprocess3d"] = timed(lambda k: ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data), n=max(3, reps // 4))
# labels: every post-pass makes a new mesh, so the labels are made again after each
out["labels"] = timed(lambda k: ctx.lib.cx_level1_component_labels(ctx.handle, ctypes.byref(lab), None), n=max(3, reps // 4),
                      before=lambda k: ctx._check(ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data)))
table = ctx.level1_components()
keep = np.ascontiguousarray((np.arange(len(table)) == int(np.argmax(table["triangles"]))).astype(np.uint8))
out["keep_largest_1"] = timed(lambda k: ctx.lib.cx_level1_keep_components(ctx.handle, keep.ctypes.data, counts.ctypes.data), n=max(3, reps // 4),
                              before=lambda k: (ctx._check(ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data)),
                                                ctx._check_attr(ctx.lib.cx_level1_component_labels(ctx.handle, ctypes.byref(lab), None))))
out["largest"] = {"triangles": int(table["triangles"].max()), "kept_vertices": int(counts[0]), "kept_triangles": int(counts[1])}
out["read_bandwidth_GB_per_s"] = round(float(ctx.measure_read_bandwidth(A.data_ptr(), A.numel() * 4, 5)), 1)     # the grid, 512 MB
out["measures_fraction_of_read_bandwidth"] = round(out["measures_call_GB_per_s"] / out["read_bandwidth_GB_per_s"], 3)
ctx.close()
line = json.dumps(out)
print(line)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_components_%d.json" % size), "w") as f:
    f.write(line + "\n")
