#!/usr/bin/env python3
"""per-call times of cx_grid_rank3d on the bench field (512^3, the bench's generator), the fp32 field and a uint8 copy of it (256 steps
between its minimum and maximum), mode "nearest", in one warm process:
  the median over 3^3, 5^3 and 7^3 and over ball(2) (33 offsets in 5^3): the general kernel;
  the minimum and the maximum over 3^3 and 7^3: the separable kernel; and the same ranks with an all-ones footprint, which the
  dispatch sends to the general kernel: what the separable path is worth, and that it grows with s0 + s1 + s2.
Beside each time:
  the traffic floor: one read plus one write of the array in its own type at the rate cx_measure_read_bandwidth reports here;
  the work floor of the general kernel: W x key bits LDS reads per output (the separable kernel: s0 + s1 + s2 reads per output before
  the halo's share);
  for the 3^3 median, scipy.ndimage.median_filter once on the host, with equality asserted (argument 3 = 0 leaves it out).
3 warm + `reps` timed calls, each between two HIP events on the context's stream; the result goes into the context's own buffer.
Prints one JSON line and writes it to profiles/bench_rank_<size>.json."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic, volume
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
with_scipy = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
dev = torch.device("cuda", 0)
F = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
n = F.numel()
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
lo, hi = float(F.min()), float(F.max())
U = ((F - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8).contiguous()
shape = tuple(int(x) for x in F.shape)


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


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n, "mode": "nearest"}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)


def case(name, box, rank, footprint=None, scipy_check=False):
    "rank: an index, or 'median' / 'max'"
    box = (box,) * 3 if np.ndim(box) == 0 else tuple(box)
    W = int(np.prod(box)) if footprint is None else int(np.sum(footprint))
    r_index = {"median": W // 2, "max": W - 1}.get(rank, rank)
    separable = footprint is None and r_index in (0, W - 1)
    for label, T in (("fp32", F), ("uint8", U)):
        samples = (T.data_ptr(), T.dtype, shape)
        r = timed(lambda: ctx.rank_grid(box, r_index, footprint, None, "nearest", 0, samples=samples))
        bits = 8 * T.element_size()
        floor_ms = 2 * n * T.element_size() / (GBps * 1e9) * 1e3
        r.update(box=list(box), W=W, rank=r_index, kernel="separable" if separable else "general", traffic_floor_ms=round(floor_ms, 4),
                 over_traffic_floor=round(r["median_ms"] / floor_ms, 2),
                 lds_reads_per_output=int(sum(box)) if separable else W * bits)
        r["ns_per_output_read"] = round(r["median_ms"] * 1e6 / (n * r["lds_reads_per_output"]), 6)
        if scipy_check and with_scipy:
            import scipy.ndimage as ndi
            host = T.cpu().numpy()
            t0 = time.time()
            want = ndi.median_filter(host, size=box, mode="nearest")
            r["scipy_median_filter_s"] = round(time.time() - t0, 2)
            got = ctx.rank_grid(box, r_index, footprint, None, "nearest", 0, samples=samples, download=True)[1]
            assert np.array_equal(got, want), "the device median differs from scipy.ndimage.median_filter"
            r["equals_scipy"] = True
            r["scipy_over_device"] = round(r["scipy_median_filter_s"] * 1e3 / r["median_ms"], 1)
        out[name + "_" + label] = r
        print(name, label, r["median_ms"], "ms", file=sys.stderr, flush=True)


case("median_3", 3, "median", scipy_check=True)
case("median_5", 5, "median")
case("median_7", 7, "median")
case("median_ball2", 5, "median", volume.ball(2))
for s in (3, 7):
    case("min_%d" % s, s, 0)
    case("max_%d" % s, s, "max")
    case("min_%d_general" % s, s, 0, np.ones((s,) * 3, dtype=bool))
    case("max_%d_general" % s, s, "max", np.ones((s,) * 3, dtype=bool))
for label in ("fp32", "uint8"):
    out["separable_7_over_3_" + label] = round(out["min_7_" + label]["median_ms"] / out["min_3_" + label]["median_ms"], 2)
    out["general_7_over_3_" + label] = round(out["min_7_general_" + label]["median_ms"] / out["min_3_general_" + label]["median_ms"], 2)
    out["general_over_separable_7_" + label] = round(out["min_7_general_" + label]["median_ms"] / out["min_7_" + label]["median_ms"], 2)
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_rank_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
