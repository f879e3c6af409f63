#!/usr/bin/env python3
"""per-call times of the rim caps on the bench field (512^3, the bench's generator and isovalue), in one warm process: cx_postprocess3d
(the plain path, the yardstick), cx_cap3d alone with all six faces, and cx_postprocess3d_capped.  3 warm + `reps` timed calls between
HIP events on the context's stream; cx_cap3d is idempotent per request, so the timed calls alternate between the two sides (each
builds its cap anew; the library's own event pair around the kernels is read back through cx_cap3d_info).
Reported next to the times: the least traffic of the cap kernels -- the lines of the six faces (an i- or j-face is contiguous samples;
every sample of a k-face sits in a 128-byte line of its own), the 8-byte vertex records once, the cap written (8 bytes per vertex
record, 12 per triangle) -- at the read rate cx_measure_read_bandwidth reports in this process, the size of the table of the rim's
crossings, and cx_device_bytes before and after the first cap.
The bench field's generator pads two layers of samples below every isovalue around the volume, so its surface never meets the rim:
the cap "above" is empty and the cap "below" is the whole box without a single crossing.  The same measurements are therefore made a
second time on the field WITHOUT that padding (its inner (size-4)^3 block as a grid of its own), where the surface runs into all six
faces: "cropped" in the output.
Prints one JSON line and writes it to profiles/bench_cap_<size>.json."""
import json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dev = torch.device("cuda", 0)
F = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)


def measure(A):
    n = int(A.shape[0])
    ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.adopt_device_grid(A.data_ptr(), tuple(A.shape), keepalive=A)
    c0 = ctx.extract3d(0.0, 1)
    post = ctx.postprocess3d(0)
    counts, k4 = np.zeros(8, dtype=np.int64), np.zeros(4, dtype=np.int64)
    read_GBps = ctx.measure_read_bandwidth(A.data_ptr(), A.numel() * 4, 5)

    def timed(call, n=reps, info=False):
        "median / min / max milliseconds of n calls after 3 warm ones, each between two events on the context's stream"
        ms, kern = [], []
        for k in range(3 + n):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx._check(call(k))
            e1.record()
            e1.synchronize()
            if k >= 3:
                ms.append(e0.elapsed_time(e1))
                if info:
                    kern.append(ctx.cap_info()["ms"])
        r = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
        if info:
            r["kernels_median_ms"] = round(statistics.median(kern), 4)
        return r

    few = max(3, reps // 4)
    out = {"shape": [n] * 3, "level0": c0, "level1": post, "read_GBps": round(read_GBps, 1)}
    out["open_components"] = int((ctx.level1_components()["closed"] == 0).sum())
    out["boundary_edges"] = int(ctx.level1_topology()["boundary_edges"].sum())
    live0 = _ffi.device_bytes(ctx.handle)[0]
    cap_counts = ctx.cap3d("all", "above")
    out["device_bytes_before_first_cap"], out["device_bytes_after_first_cap"] = live0, _ffi.device_bytes(ctx.handle)[0]
    out["cap_above"], out["cap_below"] = cap_counts, ctx.cap3d("all", "below")
    r = timed(lambda k: ctx.lib.cx_cap3d(ctx.handle, 63, k & 1, k4.ctypes.data), info=True)
    i = ctx.cap_info()
    ncv = [c["n_lattice_vertices"] + c["n_missing_crossings"] for c in (out["cap_above"], out["cap_below"])]
    nct = [c["n_cap_triangles"] for c in (out["cap_above"], out["cap_below"])]
    face_bytes = 2 * n * n * 4 + 2 * n * n * 4 + 2 * n * n * 128
    least = face_bytes + 8 * int(c0["n_vertices"]) + 8 * sum(ncv) // 2 + 12 * sum(nct) // 2          # (the mean of the two sides the calls alternate between)
    least_ms = least / (read_GBps * 1e9) * 1e3
    r.update(rim_records=i["n_rim_records"], table_slots=i["table_slots"], rim_points=i["n_rim_points"], least_traffic_bytes=int(least),
             least_traffic_ms=round(least_ms, 4), kernels_over_least=round(r["kernels_median_ms"] / least_ms, 2))
    out["cap3d_all_faces"] = r
    out["postprocess3d"] = timed(lambda k: ctx.lib.cx_postprocess3d_ex(ctx.handle, 0, 0.0, counts.ctypes.data), n=few)
    ctx.cap3d("all", "above")
    out["postprocess3d_capped"] = timed(lambda k: ctx.lib.cx_postprocess3d_capped(ctx.handle, 0, counts.ctypes.data), n=few)
    out["level1_capped"] = dict(n_vertices=int(counts[0]), n_triangles=int(counts[1]), n_components=int(counts[4]))
    out["open_components_capped"] = int((ctx.level1_components()["closed"] == 0).sum())
    out["boundary_edges_capped"] = int(ctx.level1_topology()["boundary_edges"].sum())
    out["capped_over_postprocess3d"] = round(out["postprocess3d_capped"]["median_ms"] / out["postprocess3d"]["median_ms"], 3)
    out["cap3d_over_postprocess3d"] = round(out["cap3d_all_faces"]["median_ms"] / out["postprocess3d"]["median_ms"], 3)
    out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
    ctx.close()
    return out


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0)}
out.update(measure(F))
out["cropped"] = measure(F[2:-2, 2:-2, 2:-2].contiguous())
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_cap_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
