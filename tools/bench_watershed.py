#!/usr/bin/env python3
"""per-call times of cx_grid_watershed3d on the bench field (512^3, the bench's generator), connectivity 1, in one warm process:
  split_step     split_touching's watershed step alone: a falling flood of the float32 distance() field inside {f >= median} from its
                 labelled h-maxima (h = 2 samples), with {f >= median} as the region;
  rising_fp32    a rising flood of the fp32 field from its labelled regional minima;
  rising_uint8   the same of a uint8 copy of the field (256 steps between its minimum and maximum).
Beside each time: the rounds, tile visits and doubling passes of the last call, the exact counts, and the multiple of the traffic floor:
one read of relief, markers and region plus one write of the labels at the rate cx_measure_read_bandwidth reports here.
As context only: scipy.ndimage.watershed_ift of the uint8 case on this host in seconds (its ties differ, so results are not compared;
argument 3 = 0 leaves it out), and the times of the nearest existing kernels from profiles/bench_recon_<size>.json where that exists.
3 warm + `reps` timed calls, each between two HIP events on the context's stream; the labels go into the context's own buffer.
Prints one JSON line and writes it to profiles/bench_watershed_<size>.json."""
import json, os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
with_scipy = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
dev = torch.device("cuda", 0)
F = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
n = F.numel()
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
lo, hi = float(F.min()), float(F.max())
U = ((F - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8).contiguous()
shape = tuple(int(x) for x in F.shape)
median = float(F.view(-1).kthvalue(n // 2 + 1).values)


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


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n, "connectivity": 1, "median": median, "h": 2.0,
       "hardware_counters_read": False}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)


def labelled_extrema(T, method):
    "the labelled regional extrema of T as an int32 tensor, and how many"
    _, mask = ctx.reconstruct_grid("step", method=method, out_kind="changed", samples=(T.data_ptr(), T.dtype, shape))
    labels = torch.empty(shape, dtype=torch.int32, device=dev)
    k, _ = ctx.label_grid(0.5, "high", 1, samples=(mask, "uint8", shape), out=labels.data_ptr())
    return labels, k


def case(name, T, markers, k, region, direction):
    samples = (T.data_ptr(), T.dtype, shape)
    last = {}

    def call():
        last["stats"] = ctx.watershed_grid(markers.data_ptr(), None if region is None else region.data_ptr(), 1, direction, samples=samples)[0]
    r = timed(call)
    floor_ms = n * (T.element_size() + 4 + (0 if region is None else 1) + 4) / (GBps * 1e9) * 1e3
    r.update(last["stats"])
    r.update(labels=int(k), direction=direction, traffic_floor_ms=round(floor_ms, 4), over_traffic_floor=round(r["median_ms"] / floor_ms, 2),
             tiles=int(np.prod([-(-s // t) for s, t in zip(shape, (8, 8, 64))])))
    out[name] = r
    print(name, r["median_ms"], "ms", r["rounds"], "rounds", r["jump_rounds"], "doubling passes", file=sys.stderr, flush=True)
    return r


def write():
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_watershed_%d.json" % size), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


D = torch.empty(shape, dtype=torch.float32, device=dev)
ctx.distance_grid(median, "above", "float32", samples=(F.data_ptr(), F.dtype, shape), out=D.data_ptr())
H = torch.empty(shape, dtype=torch.float32, device=dev)
ctx.reconstruct_grid("shift", h=out["h"], samples=(D.data_ptr(), D.dtype, shape), out=H.data_ptr())
markers, k = labelled_extrema(H, "dilation")
del H
region = (F >= median).to(torch.uint8).contiguous()
torch.cuda.synchronize()
case("split_step", D, markers, k, region, "falling")
del D, region, markers
markers, k = labelled_extrema(F, "erosion")
torch.cuda.synchronize()
case("rising_fp32", F, markers, k, None, "rising")
markers, k = labelled_extrema(U, "erosion")
torch.cuda.synchronize()
case("rising_uint8", U, markers, k, None, "rising")
recon = os.path.join(ROOT, "profiles", "bench_recon_%d.json" % size)
if os.path.exists(recon):      # the nearest existing kernels, as context
    with open(recon) as f:
        prior = json.load(f)
    out["context_bench_recon"] = {name: {key: prior[name][key] for key in ("median_ms", "rounds", "tile_visits") if key in prior[name]}
                                  for name in ("regional_maxima_of_distance", "propagate_uint8") if name in prior}
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
write()
if with_scipy:
    import scipy.ndimage as ndi
    relief_h, markers_h = U.cpu().numpy(), markers.cpu().numpy()
    t0 = time.time()
    ndi.watershed_ift(relief_h, markers_h)
    out["rising_uint8"]["scipy_watershed_ift_s"] = round(time.time() - t0, 2)      # (not compared: the ties differ)
    write()
ctx.close()
print(json.dumps(out))
