#!/usr/bin/env python3
"""per-call times of the connected-component labelling (cx_grid_label3d, csrc/cx_label.hip) at 512^3, in one warm process:
  (a) the bench field (the bench's generator) thresholded at its median (levels.quantiles, 0.5): few large components;
  (b) uniform noise thresholded so that half of the samples are labelled, and so that 31 % are: about two million components, the
      second at the percolation threshold of 6-connectivity, where the unions are hardest;
each as fp32 samples and as a uint8 copy, side "high", at connectivity 1 and 3.
Beside each time:
  K;
  the floor: one streaming read of the input in its own type plus one write of the int32 labels, at the rate
  cx_measure_read_bandwidth reports here;
  the time of every kernel of the call (the five of cx_label.hip and the three of the scan), from the device-side kernel records of
  torch.profiler over `reps` further calls, where the profiler gives any;
  for the fp32 cases of connectivity 1 the records (cx_grid_label3d_measures, first request) and a select (cx_grid_label3d_select);
  for case (a), fp32, connectivity 1: scipy.ndimage.label on the host, where scipy imports (once), and whether the labels are equal.
3 warm + `reps` timed calls, each between two HIP events on the context's stream; the labels go into the context's own buffer.
Prints one JSON line and writes it to profiles/bench_label_<size>.json."""
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
KERNELS = ("cxl_k_rows", "cxl_k_unite", "cxl_k_flatten", "cxp_k_scan_blocks", "cxp_k_scan_sums", "cxp_k_scan_add", "cxl_k_relabel")


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


def kernel_times(call):
    "mean milliseconds per call of every kernel of KERNELS, from the profiler's device-side records; a string when it gives none"
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        found = {}
        for ev in prof.key_averages():
            for name in KERNELS:
                if name in ev.key:
                    total_us = getattr(ev, "device_time_total", None)
                    if total_us is None:
                        total_us = ev.cuda_time_total
                    found[name] = round(found.get(name, 0.0) + total_us / 1e3 / reps, 4)
        return found if found else "not measured: the profiler recorded no kernel"
    except Exception as e:      # a profiler that does not start must not cost the call times
        return "not measured: %s" % type(e).__name__


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)


def case(name, T, value, connectivity, extras=False, scipy_of=False):
    shape = tuple(int(x) for x in T.shape)
    samples = (T.data_ptr(), T.dtype, shape)
    k, _ = ctx.label_grid(value, "high", connectivity, samples=samples)
    r = timed(lambda: ctx.label_grid(value, "high", connectivity, samples=samples))
    in_bytes, out_bytes = T.numel() * T.element_size(), T.numel() * 4
    floor_ms = (in_bytes + out_bytes) / (GBps * 1e9) * 1e3
    r.update(value=value, connectivity=connectivity, dtype=str(T.dtype).replace("torch.", ""), n_components=k, input_bytes=in_bytes,
             output_bytes=out_bytes, floor_ms=round(floor_ms, 4), over_floor=round(r["median_ms"] / floor_ms, 2))
    r["kernel_ms"] = kernel_times(lambda: ctx.label_grid(value, "high", connectivity, samples=samples))
    if extras:
        def first_measures():
            ctx.label_grid(value, "high", connectivity, samples=samples)
            ctx.label_measures()
        both = timed(first_measures, max(3, reps // 2))
        r["label_and_measures_ms"] = both["median_ms"]
        r["measures_ms"] = round(both["median_ms"] - r["median_ms"], 4)
        keep = (np.arange(k + 1) % 2).astype(np.uint8)
        r["select_ms"] = timed(lambda: ctx.label_select(keep))["median_ms"]
        r["select_floor_ms"] = round((n * 4 + n) / (GBps * 1e9) * 1e3, 4)
    if scipy_of and with_scipy:
        try:
            from scipy import ndimage
            host = T.cpu().numpy()
            t0 = time.perf_counter()
            ref, k_ref = ndimage.label(host >= value, ndimage.generate_binary_structure(3, connectivity))
            r["scipy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            mine = ctx.label_grid(value, "high", connectivity, samples=samples, download=True)[1]
            r["equals_scipy"] = bool(k_ref == k and np.array_equal(mine, ref))
            r["scipy_over_device"] = round(r["scipy_host_ms"] / r["median_ms"], 1)
        except ImportError:
            r["scipy_host_ms"] = "not measured: scipy does not import"
    out[name] = r


def as_uint8(T):
    lo, hi = float(T.min()), float(T.max())
    return ((T - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8).contiguous()


U = as_uint8(F)
vF = float(levels.quantiles(F, 0.5)[0])
vU = float(levels.quantiles(U, 0.5)[0]) + 0.5
N = torch.rand((size,) * 3, generator=torch.Generator(device=dev).manual_seed(1236), device=dev, dtype=torch.float32)
NU = as_uint8(N)
for c in (1, 3):
    case("median_fp32_c%d" % c, F, vF, c, extras=c == 1, scipy_of=c == 1)
    case("median_uint8_c%d" % c, U, vU, c)
    for density in (0.5, 0.31):
        tag = "noise%02d" % round(density * 100)
        case("%s_fp32_c%d" % (tag, c), N, 1.0 - density, c, extras=c == 1)
        case("%s_uint8_c%d" % (tag, c), NU, float(levels.quantiles(NU, 1.0 - density)[0]) + 0.5, c)
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_label_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
