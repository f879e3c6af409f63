#!/usr/bin/env python3
"""per-call times of preparing the volume on the bench field (512^3, the bench's generator), in one warm process:
  gaussian sigma 1 (9 taps per axis) of the fp32 field and of a uint8 copy of it (256 steps between its minimum and maximum);
  gaussian sigma 2 (17 taps) at stride 2; one pyramid step ([1, 4, 6, 4, 1] / 16 at stride 2), both of the fp32 field.
Beside each time:
  the floor: one streaming read of the input in its own type plus one write of the fp32 output, at the rate
  cx_measure_read_bandwidth reports here;
  the bytes the two kernels request by construction (csrc/cx_filter.hip): a wave of the first kernel reads (r - 1) stride + taps
  input rows of 63 stride + taps samples for r rows of 64 outputs and writes them, r = 16 or as many as keep those rows within its
  window of 32; a wave of the second reads (r - 1) stride + taps rows of 64 for r and writes them.  Rows and halos that neighbouring waves read again count every time, wherever they are served from;
  the host time of scipy.ndimage.gaussian_filter where scipy imports (sigma 1 only, once each).
3 warm + `reps` timed calls, each between two HIP events on the context's stream; the result goes into the context's own buffer.
Prints one JSON line and writes it to profiles/bench_filter_<size>.json."""
import json, os, statistics, sys, time
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
ctx.adopt_device_grid(F.data_ptr(), tuple(F.shape), keepalive=F)
lo, hi = float(F.min()), float(F.max())
U = ((F - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8).contiguous()
R, LANES, WINDOW = 16, 64, 32      # CXF_R, columns of a wave, CXF_WROWS


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


def requested_bytes(shape, itemsize, axes):
    "what the kernels load and store by construction: {first kernel read, first kernel write, second kernel read, second kernel write}"
    (w0, _, s0), (w1, _, s1), (w2, _, s2) = axes
    t0, t1, t2 = (0 if w is None else len(w) for w in (w0, w1, w2))
    m = [-(-shape[a] // s) for a, s in enumerate((s0, s1, s2))]
    planes = shape[0] if t0 else m[0]

    def walked(taps, stride, outputs):      # input rows read for `outputs` outputs along a walked axis
        taps = max(taps, 1)
        rc = R      # outputs per wave: as many as keep its rows within the window (cxf_chunking)
        if taps <= WINDOW:
            rc = min(R, (WINDOW - taps) // stride + 1 if stride < taps else WINDOW // taps)
        chunks, last = divmod(outputs, rc)
        per = lambda rv: ((rv - 1) * stride + taps) if stride < taps else rv * taps
        return chunks * per(rc) + (per(last) if last else 0)

    def row_samples(taps, stride, outputs):      # samples read of one input row for `outputs` columns
        taps = max(taps, 1)
        tiles, last = divmod(outputs, LANES)
        per = lambda nc: ((nc - 1) * stride + taps) if stride < taps else nc * taps
        return tiles * per(LANES) + (per(last) if last else 0)

    k1_read = planes * walked(t1, s1, m[1]) * row_samples(t2, s2, m[2]) * itemsize
    k1_write = planes * m[1] * m[2] * 4
    k2_read = walked(t0, s0, m[0]) * m[1] * m[2] * 4 if t0 else 0
    k2_write = m[0] * m[1] * m[2] * 4 if t0 else 0
    return {"rows_kernel_read": k1_read, "rows_kernel_write": k1_write, "planes_kernel_read": k2_read, "planes_kernel_write": k2_write,
            "total": k1_read + k1_write + k2_read + k2_write}


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)


def case(name, T, axes, scipy_sigma=None):
    shape = tuple(int(x) for x in T.shape)
    samples = (T.data_ptr(), T.dtype, shape)
    got, _ = ctx.filter_grid(axes, "nearest", 0.0, samples=samples)
    r = timed(lambda: ctx.filter_grid(axes, "nearest", 0.0, samples=samples))
    in_bytes, out_bytes = T.numel() * T.element_size(), int(np.prod(got)) * 4
    floor_ms = (in_bytes + out_bytes) / (GBps * 1e9) * 1e3
    moved = requested_bytes(shape, T.element_size(), axes)
    r.update(result_shape=list(got), taps=[0 if w is None else len(w) for w, _, _ in axes], strides=[s for _, _, s in axes],
             input_bytes=in_bytes, output_bytes=out_bytes, floor_ms=round(floor_ms, 4), over_floor=round(r["median_ms"] / floor_ms, 2),
             requested_bytes=moved, requested_over_floor_bytes=round(moved["total"] / (in_bytes + out_bytes), 2),
             requested_GBps=round(moved["total"] / (r["median_ms"] * 1e-3) / 1e9, 1))
    if scipy_sigma is not None:
        try:
            from scipy import ndimage
            host = T.cpu().numpy()
            t0 = time.perf_counter()
            ref = ndimage.gaussian_filter(host, scipy_sigma, output=np.float32, mode="nearest")
            r["scipy_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            mine = ctx.filter_grid(axes, "nearest", 0.0, samples=samples, download=True)[1]
            r["max_abs_difference_from_scipy"] = float(np.abs(mine - ref).max())
            r["scipy_over_device"] = round(r["scipy_host_ms"] / r["median_ms"], 1)
        except ImportError:
            r["scipy_host_ms"] = "not measured: scipy does not import"
    out[name] = r


def gauss(sigma, stride):
    w = volume.gaussian_weights(sigma)
    return [(w, len(w) // 2, stride)] * 3


case("gaussian_sigma1_fp32", F, gauss(1.0, 1), scipy_sigma=1.0)
case("gaussian_sigma1_uint8", U, gauss(1.0, 1), scipy_sigma=1.0)
case("gaussian_sigma2_stride2_fp32", F, gauss(2.0, 2))
pw = np.asarray(volume.PYRAMID_WEIGHTS, dtype=np.float32)
case("pyramid_step_fp32", F, [(pw, 2, 2)] * 3)
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_filter_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
