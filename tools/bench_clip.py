#!/usr/bin/env python3
"""per-call times of the clip of the Level-1 mesh on the bench field (512^3, the bench's generator and isovalue): an oblique plane
through the volume's centre, the plane x = size/2 (many vertices exactly on it), and a clip by a second field, next to
cx_postprocess3d and cx_level1_simplify (cell 4) of the same mesh in the same process.  Warm context, 3 warm + `reps` timed calls
between HIP events on the context's stream; the clip's own kernels and its tail (clean, compaction, orientation, map) are timed
separately by the library (cx_level1_clip_info).  A clip consumes its input, so every timed call is preceded by an untimed
cx_postprocess3d (and, for the field, by the sampling of the second grid, which is timed on its own).
Reported next to the times: the minimum traffic of the clip kernels (the triangles read once, the two vertex bit masks, points and
scalars of both ends of every cut edge, the output triangles written) at the read rate cx_measure_read_bandwidth reports in this
process, the size of the edge table against the cut corners, and cx_device_bytes before and after the first clip.
Prints one JSON line and writes it to profiles/bench_clip_<size>.json."""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
A = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
B = synthetic.smooth_noise_torch((size,) * 3, 4321, 1400, dev)          # the second field of the field= clip
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.adopt_device_grid(A.data_ptr(), tuple(A.shape), keepalive=A)
ctx.extract3d(0.0, 1)
post = ctx.postprocess3d(0)
counts, cc, sc, q = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64), ctypes.c_double(0.0)
vals, lab = ctypes.c_void_p(), ctypes.c_void_p()
read_GBps = ctx.measure_read_bandwidth(A.data_ptr(), A.numel() * 4, 5)


def restore(k):
    ctx._check(ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data))


def sample(k):
    return ctx.lib.cx_level1_sample_grid(ctx.handle, ctypes.c_void_p(B.data_ptr()), 0, 1, ctypes.byref(vals), None)


def timed(call, n=reps, before=None, info=False):
    "median / min / max milliseconds of n calls after 3 warm ones, each between two events on the context's stream"
    ms, kern, tail = [], [], []
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
            if info:
                i = ctx.level1_clip_info()
                kern.append(i["kernels_ms"]); tail.append(i["tail_ms"])
    out = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
    if info:
        out.update(kernels_median_ms=round(statistics.median(kern), 4), tail_median_ms=round(statistics.median(tail), 4))
    return out


def clip_case(name, call, before):
    r = timed(call, n=few, before=before, info=True)
    i = ctx.level1_clip_info()
    nv, nt = i["n_vertices_before"], i["n_triangles_before"]
    # the least the clip kernels could move: triangles in, two bit masks, {point, scalar} of both ends of every cut edge, triangles out
    least = 12 * nt + 2 * ((nv + 7) // 8) + int(cc[2]) * 2 * (24 + 8) + 12 * i["n_raw_triangles"]
    least_ms = least / (read_GBps * 1e9) * 1e3
    r.update(vertices=int(cc[0]), triangles=int(cc[1]), cut_vertices=int(cc[2]), cut_triangles=int(cc[3]), on_cut=int(cc[6]), raw_triangles=int(cc[7]),
             cut_corners=i["cut_corners"], table_slots=i["table_slots"], table_slots_if_sized_by_the_mesh=int(_table_size(3 * nt)),
             least_traffic_bytes=int(least), least_traffic_ms=round(least_ms, 4), kernels_over_least=round(r["kernels_median_ms"] / least_ms, 2),
             tail_share=round(r["tail_median_ms"] / (r["tail_median_ms"] + r["kernels_median_ms"]), 3))
    out[name] = r


def _table_size(n):
    s = 1024
    while s < 2 * n + 16:
        s <<= 1
    return s


few = max(3, reps // 4)
out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "level1": post, "read_GBps": round(read_GBps, 1)}
live0 = _ffi.device_bytes(ctx.handle)[0]
c = 0.5 * (size - 1)
n = np.array([0.36, 0.48, 0.8])
p_oblique = np.ascontiguousarray(np.concatenate([n, [float(n @ np.array([c, c, c]))]]))
p_x = np.ascontiguousarray(np.array([1.0, 0.0, 0.0, float(size // 2)]))
ctx._check_attr(ctx.lib.cx_level1_clip_plane(ctx.handle, p_oblique.ctypes.data, 0, cc.ctypes.data))
out["device_bytes_before_first_clip"], out["device_bytes_after_first_clip"] = live0, _ffi.device_bytes(ctx.handle)[0]
clip_case("plane_oblique", lambda k: ctx.lib.cx_level1_clip_plane(ctx.handle, p_oblique.ctypes.data, 0, cc.ctypes.data), restore)
clip_case("plane_oblique_no_clean", lambda k: ctx.lib.cx_level1_clip_plane(ctx.handle, p_oblique.ctypes.data, _ffi.CX_CLIP_NO_CLEAN, cc.ctypes.data), restore)


def restore_normals(k):
    restore(k)
    ctx._check_attr(ctx.lib.cx_level1_normals(ctx.handle, None, ctypes.byref(lab)))


clip_case("plane_oblique_normals", lambda k: ctx.lib.cx_level1_clip_plane(ctx.handle, p_oblique.ctypes.data, _ffi.CX_CLIP_NORMALS, cc.ctypes.data), restore_normals)
clip_case("plane_x_half", lambda k: ctx.lib.cx_level1_clip_plane(ctx.handle, p_x.ctypes.data, 0, cc.ctypes.data), restore)


def restore_sampled(k):
    restore(k)
    ctx._check_attr(sample(k))


clip_case("field", lambda k: ctx.lib.cx_level1_clip_scalars(ctx.handle, vals, 1, 0.0, 0, cc.ctypes.data), restore_sampled)
restore(0)
out["sample_grid"] = timed(sample)
out["postprocess3d"] = timed(lambda k: ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data), n=few)
c3 = np.array([4.0, 4.0, 4.0], dtype=np.float64)
out["simplify_cell_4"] = timed(lambda k: ctx.lib.cx_level1_simplify(ctx.handle, c3.ctypes.data, 0, sc.ctypes.data, ctypes.byref(q)), n=few,
                               before=lambda k: (restore(k), ctx._check_attr(ctx.lib.cx_level1_component_labels(ctx.handle, None, ctypes.byref(lab)))))
out["plane_oblique_over_postprocess3d"] = round(out["plane_oblique"]["median_ms"] / out["postprocess3d"]["median_ms"], 3)
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_clip_%d.json" % size), "w") as f:
    f.write(line + "\n")
