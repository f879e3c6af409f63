#!/usr/bin/env python3
"""per-call times of the exact Euclidean distance transform (cx_grid_distance3d, csrc/cx_dist.hip) at 512^3, in one warm process:
  (a) the bench field (the bench's generator) thresholded at its median (levels.quantiles, 0.5), as fp32 samples and as a uint8 copy
      (256 steps between its minimum and maximum, thresholded at the copy's own median): side "signed" with float32 output, and side
      "below" with mask output at radius 3;
  (b) the same shape with a single site in a corner: the worst case for a pruned search.
Beside each time:
  the floor: one streaming read of the input in its own type plus one write of the result, at the rate cx_measure_read_bandwidth
  reports here;
  the bytes the three kernels request: the fixed part by construction (the first kernel reads the samples once and a double per sample
  once, and writes a double per sample twice; each of the other two reads its own sample's double and writes one value), and a lower
  bound of the searches' part, computed from the result: a lane scans in rounds of 4 distances (8 doubles) while w d^2 of the round's
  first distance is below its best so far, which is at least its final squared distance, and at most to the far end of the axis;
  the host time of scipy.ndimage.distance_transform_edt for case (a) where scipy imports (once each).
3 warm + `reps` timed calls, each between two HIP events on the context's stream; the result goes into the context's own buffer.
Prints one JSON line and writes it to profiles/bench_distance_<size>.json."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, levels, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
with_scipy = "--no-scipy" not in sys.argv
dev = torch.device("cuda", 0)
F = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
n = F.numel()
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
lo, hi = float(F.min()), float(F.max())
U = ((F - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8).contiguous()
BATCH = 4      # CXD_BATCH


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


def search_rounds_lower_bound(T, value):
    "rounds of the outward scans of the two walking kernels, at least: from the squared distance of every sample to the other class"
    shape = tuple(int(x) for x in T.shape)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    ctx.distance_grid(value, "signed", "squared", samples=(T.data_ptr(), T.dtype, shape), out=out.data_ptr())
    best = out.abs_()
    total = 0
    for axis in (1, 0):
        pos = torch.arange(shape[axis], device=dev, dtype=torch.float64)
        reach = torch.maximum(pos, shape[axis] - 1 - pos).reshape([-1 if a == axis else 1 for a in range(3)])
        # rounds start at d0 = 1, 5, 9, ...: those with d0^2 < best and d0 <= reach
        far = torch.minimum(torch.ceil(torch.sqrt(best)) - 1, reach)      # the largest d0 that may start a round
        total += int(torch.ceil(far.clamp_(min=0) / BATCH).sum().item())
    return total


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)
KIND_BYTES = {"squared": 8, "float32": 4, "mask": 1}


def case(name, T, value, side, kind, radius2=0.0, rounds=None, scipy_of=None):
    shape = tuple(int(x) for x in T.shape)
    samples = (T.data_ptr(), T.dtype, shape)
    sites, _ = ctx.distance_grid(value, side, kind, None, radius2, samples=samples)
    r = timed(lambda: ctx.distance_grid(value, side, kind, None, radius2, samples=samples))
    in_bytes, out_bytes = T.numel() * T.element_size(), T.numel() * KIND_BYTES[kind]
    floor_ms = (in_bytes + out_bytes) / (GBps * 1e9) * 1e3
    fixed = in_bytes + 3 * 8 * n + (8 * n + 8 * n) + (8 * n + out_bytes)
    moved = {"fixed": fixed, "searches_at_least": None if rounds is None else rounds * 2 * BATCH * 8}
    moved["total_at_least"] = fixed + (moved["searches_at_least"] or 0)
    r.update(value=value, side=side, kind=kind, radius2=radius2, n_sites=sites, input_bytes=in_bytes, output_bytes=out_bytes,
             floor_ms=round(floor_ms, 4), over_floor=round(r["median_ms"] / floor_ms, 2), requested_bytes=moved,
             requested_over_floor_bytes=round(moved["total_at_least"] / (in_bytes + out_bytes), 2),
             requested_GBps_at_least=round(moved["total_at_least"] / (r["median_ms"] * 1e-3) / 1e9, 1))
    if scipy_of is not None and with_scipy:
        try:
            from scipy import ndimage
            host = T.cpu().numpy()
            t0 = time.perf_counter()
            low = host < value
            ref = ndimage.distance_transform_edt(~low) - ndimage.distance_transform_edt(low)
            r["scipy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            mine = ctx.distance_grid(value, side, kind, None, radius2, samples=samples, download=True)[1]
            r["equals_scipy_rounded_to_float32"] = bool(np.array_equal(mine, ref.astype(np.float32)))
            r["scipy_over_device"] = round(r["scipy_host_ms"] / r["median_ms"], 1)
        except ImportError:
            r["scipy_host_ms"] = "not measured: scipy does not import"
    out[name] = r


vF = float(levels.quantiles(F, 0.5)[0])
vU = float(levels.quantiles(U, 0.5)[0]) + 0.5
rF, rU = search_rounds_lower_bound(F, vF), search_rounds_lower_bound(U, vU)
case("median_signed_float32_fp32", F, vF, "signed", "float32", rounds=rF, scipy_of=True)
case("median_signed_float32_uint8", U, vU, "signed", "float32", rounds=rU, scipy_of=True)
case("median_dilate_radius3_fp32", F, vF, "below", "mask", 9.0, rounds=rF)
case("median_dilate_radius3_uint8", U, vU, "below", "mask", 9.0, rounds=rU)
S = torch.zeros((size,) * 3, dtype=torch.uint8, device=dev)
S[size - 1, 0, size - 1] = 1
rS = search_rounds_lower_bound(S, 0.5)
case("single_site_signed_float32_uint8", S, 0.5, "signed", "float32", rounds=rS)
case("single_site_dilate_radius3_uint8", S, 0.5, "below", "mask", 9.0, rounds=rS)
out["single_site_over_median"] = round(out["single_site_signed_float32_uint8"]["median_ms"] / out["median_signed_float32_uint8"]["median_ms"], 1)
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_distance_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
