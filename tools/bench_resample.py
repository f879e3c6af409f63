#!/usr/bin/env python3
"""per-call times of cx_grid_resample3d on the bench field (512^3, the bench's generator), the fp32 field and a uint8 copy of it (256
steps between its minimum and maximum), order 1, mode "nearest", in one warm process:
  identity; zoom x2 of the inner half (256^3 -> 512^3); zoom x0.5 (-> 256^3); regrid to isotropic steps from (1, 1, 2.5) spacing
  (-> 512 x 512 x 1278); a 30 degree rotation about each axis and about (1, 1, 1), about the centre; one 512 x 512 oblique reslice.
Beside each time:
  the floor: one read of the touched input in its own type plus one write of the result, at the rate cx_measure_read_bandwidth reports
  here.  Touched input is an estimate: the outputs whose coordinates lie inside the array times |det matrix| samples (a map of
  determinant d spreads one output over d samples), at most the whole array; for the reslice (determinant 0) eight samples per output;
  torch.nn.functional.grid_sample (trilinear, align_corners=True, padding_mode="border") on the same map with its sampling grid built
  beforehand -- the yardstick from outside; it computes in fp32 and is not comparable bit for bit, so the time only.  For the uint8
  copy its time includes the conversion to fp32 it needs.
3 warm + `reps` timed calls, each between two HIP events on the context's stream; the result goes into the context's own buffer.
Prints one JSON line and writes it to profiles/bench_resample_<size>.json."""
import json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic, volume
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device("cuda", 0)
F = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
n = F.numel()
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
lo, hi = float(F.min()), float(F.max())
U = ((F - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8).contiguous()


def timed(call, count=reps):
    "median / min / max milliseconds of `count` calls after 3 warm ones, each between two events on the context's stream"
    ms = []
    for k in range(3 + count):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        if k >= 3:
            ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def rotation(axis, degrees):
    th = np.deg2rad(degrees)
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def about_centre(M, out_shape):
    c_in, c_out = (np.asarray(F.shape, dtype=np.float64) - 1.0) / 2.0, (np.asarray(out_shape, dtype=np.float64) - 1.0) / 2.0
    return M, c_in - M @ c_out


def sampling_grid(M, off, out_shape):
    "grid_sample's grid for the same map: (1, m0, m1, m2, 3) fp32, x along the last input axis, normalised so that -1 and 1 are the end samples"
    idx = [torch.arange(m, dtype=torch.float64, device=dev) for m in out_shape]
    parts = []
    for a in (2, 1, 0):
        c = off[a] + M[a, 0] * idx[0][:, None, None] + M[a, 1] * idx[1][None, :, None] + M[a, 2] * idx[2][None, None, :]
        parts.append((c * (2.0 / (F.shape[a] - 1)) - 1.0).float())
    return torch.stack(parts, dim=-1)[None].contiguous()


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n, "order": 1, "mode": "nearest"}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)


def case(name, M, off, out_shape):
    M, off = np.asarray(M, dtype=np.float64), np.asarray(off, dtype=np.float64)
    out_shape = tuple(int(m) for m in out_shape)
    count = int(np.prod(out_shape))
    det = abs(float(np.linalg.det(M)))
    grid = sampling_grid(M, off, out_shape)
    for label, T in (("fp32", F), ("uint8", U)):
        samples = (T.data_ptr(), T.dtype, tuple(int(x) for x in T.shape))
        n_outside, _ = ctx.resample_grid(M, off, out_shape, 1, "nearest", 0.0, samples=samples)
        r = timed(lambda: ctx.resample_grid(M, off, out_shape, 1, "nearest", 0.0, samples=samples))
        inside = count - n_outside
        touched = min(n, int(inside * det)) if det > 0.0 else min(n, inside * 8)
        in_bytes, out_bytes = touched * T.element_size(), count * 4
        floor_ms = (in_bytes + out_bytes) / (GBps * 1e9) * 1e3
        if label == "fp32":
            ref = lambda: torch.nn.functional.grid_sample(T[None, None], grid, mode="bilinear", padding_mode="border", align_corners=True)
        else:
            ref = lambda: torch.nn.functional.grid_sample(T[None, None].float(), grid, mode="bilinear", padding_mode="border", align_corners=True)
        g = timed(ref)
        r.update(result_shape=list(out_shape), n_outside=n_outside, determinant=round(det, 6), touched_input_bytes=in_bytes, output_bytes=out_bytes,
                 floor_ms=round(floor_ms, 4), over_floor=round(r["median_ms"] / floor_ms, 2), grid_sample_ms=g["median_ms"],
                 grid_sample_over_device=round(g["median_ms"] / r["median_ms"], 2))
        out[name + "_" + label] = r
    del grid
    torch.cuda.empty_cache()


half = size // 2
case("identity", np.eye(3), np.zeros(3), F.shape)
case("zoom2_inner_half", np.diag([0.5] * 3), np.full(3, half / 2.0 + 0.5 * 0.5 - 0.5), F.shape)
diag, off, shape = volume.zoom_map(tuple(F.shape), 0.5)
case("zoom_half", np.diag(diag), off, shape)
iso_shape = (size, size, int(round((size - 1) * 2.5)) + 1)
M, off = volume.regrid_map([0.0] * 3, [1.0, 1.0, 2.5], iso_shape, [0.0] * 3, 1.0)
case("regrid_isotropic_from_1_1_2p5", M, off, iso_shape)
for name, axis in (("rotate30_axis0", (1, 0, 0)), ("rotate30_axis1", (0, 1, 0)), ("rotate30_axis2", (0, 0, 1)), ("rotate30_diagonal", (1, 1, 1))):
    case(name, *about_centre(rotation(axis, 30.0), F.shape), F.shape)
# the plane through the centre spanned by two turned axes, 512 x 512 samples one step apart
Rm = rotation((1, 1, 1), 30.0)
u, v = Rm[:, 1], Rm[:, 2]
centre = (np.asarray(F.shape, dtype=np.float64) - 1.0) / 2.0
Mr = np.zeros((3, 3))
Mr[:, 1], Mr[:, 2] = u, v
case("reslice_oblique_%dx%d" % (size, size), Mr, centre - (u + v) * (size - 1) / 2.0, (1, size, size))
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_resample_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
