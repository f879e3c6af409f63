#!/usr/bin/env python3
"""per-call times of choosing isovalues on the bench field (512^3, the bench's generator), in one warm process:
  cx_samples_select for the 9 deciles, on the fp32 field and on a uint8 copy of it (256 steps between its minimum and maximum);
  cx_level_spectrum3d of the fp32 field at 8, 256 and 4096 levels spread evenly between the 1st and the 99th percentile (the 1st
  is the value the generator pads the volume with), and at 8 levels between the 5th and the 95th;
  the floor per pass: the time of one streaming read of the same bytes at the rate cx_measure_read_bandwidth reports here;
  what a caller does today: torch.sort of the flattened tensor followed by indexing at the same ranks.
3 warm + `reps` timed calls, each between two HIP events on the context's stream (a call ends in a device-to-host copy of its
counts, so the events enclose all of it).  The deciles are checked against the sort's, and the 8-level spectrum against 8 marches
wherever no sample lies inside a level's screen.
Prints one JSON line and writes it to profiles/bench_isovalues_<size>.json."""
import json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
dev = torch.device("cuda", 0)
F = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
n = F.numel()
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
ctx.adopt_device_grid(F.data_ptr(), tuple(F.shape), keepalive=F)


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


def floor(nbytes, ptr):
    GBps = ctx.measure_read_bandwidth(ptr, nbytes, 5)
    return {"read_GBps": round(GBps, 1), "one_pass_ms": round(nbytes / (GBps * 1e9) * 1e3, 4)}


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n}
ranks = np.floor(np.arange(1, 10) / 10.0 * (n - 1)).astype(np.int64)
flat = F.reshape(-1)

# fp32: select, the floor, the sort
deciles, n_nan = ctx.samples_select(ranks)
r = timed(lambda: ctx.samples_select(ranks))
r.update(floor(n * 4, F.data_ptr()), passes_at_least=3, deciles=[float(v) for v in deciles], n_nan=n_nan)
r["over_three_passes"] = round(r["median_ms"] / (3 * r["one_pass_ms"]), 2)
out["select_deciles_fp32"] = r
rk = torch.from_numpy(ranks).to(dev)
by_sort = torch.sort(flat).values[rk].cpu().numpy().astype(np.float64)
out["select_equals_sort_fp32"] = bool(np.array_equal(by_sort, deciles))
out["torch_sort_fp32"] = timed(lambda: torch.sort(flat).values[rk].cpu(), count=max(3, reps // 3))
out["torch_sort_over_select_fp32"] = round(out["torch_sort_fp32"]["median_ms"] / r["median_ms"], 2)

# uint8 copy
lo, hi = float(flat.min()), float(flat.max())
U = ((F - lo) * (255.0 / (hi - lo))).round().clamp(0, 255).to(torch.uint8).contiguous()
d8, _ = ctx.samples_select(ranks, int(U.data_ptr()), dtype=U.dtype, n=n)
r = timed(lambda: ctx.samples_select(ranks, int(U.data_ptr()), dtype=U.dtype, n=n))
r.update(floor(n, U.data_ptr()), passes_at_least=1, deciles=[float(v) for v in d8])
r["over_one_pass"] = round(r["median_ms"] / r["one_pass_ms"], 2)
out["select_deciles_uint8"] = r
uflat = U.reshape(-1)
out["select_equals_sort_uint8"] = bool(np.array_equal(torch.sort(uflat).values[rk].cpu().numpy().astype(np.float64), d8))
out["torch_sort_uint8"] = timed(lambda: torch.sort(uflat).values[rk].cpu(), count=max(3, reps // 3))
del U, uflat

# spectrum.  The generator pads the volume with two layers of one low value (2.3 % of the samples): the 1st percentile IS that value, so
# the first level of these sets has millions of samples inside its screen, all in one bucket.  "inner": 8 levels between the 5th and
# the 95th percentile, where the screens hold a few thousand samples
p01, p05, p95, p99 = (float(v) for v in ctx.samples_select([int(q * (n - 1)) for q in (0.01, 0.05, 0.95, 0.99)])[0])
one_pass = out["select_deciles_fp32"]["one_pass_ms"]
values = np.linspace(p05, p95, 8)
S = ctx.level_spectrum3d(values)
r = timed(lambda: ctx.level_spectrum3d(values), count=max(3, reps // 2))
r.update(levels=8, over_one_pass=round(r["median_ms"] / one_pass, 2), samples_inside_screens=int(S["n_near"].sum()))
out["spectrum_8_inner"] = r
for K in (8, 256, 4096):
    values = np.linspace(p01, p99, K)
    S = ctx.level_spectrum3d(values)
    r = timed(lambda: ctx.level_spectrum3d(values), count=max(3, reps // 2))
    r.update(levels=K, over_one_pass=round(r["median_ms"] / one_pass, 2), max_triangles=int(S["n_triangles"].max()),
             levels_with_near_samples=int((S["n_near"] > 0).sum()), samples_inside_screens=int(S["n_near"].sum()))
    out["spectrum_%d" % K] = r
    if K == 8:
        ctx.reserve(int(S["n_cells"].max()) + 4096, int(S["n_vertices"].max()) + 4096, int(S["n_triangles"].max()) + 4096)   # the curve sizes the buffers
        marched = [ctx.extract3d(float(v), 1) for v in values]
        out["spectrum_8_equals_march"] = bool(all(S["n_near"][l] > 0 or (c["n_cells"], c["n_vertices"], c["n_triangles"]) ==
                                                  (S["n_cells"][l], S["n_vertices"][l], S["n_triangles"][l]) for l, c in enumerate(marched)))
        out["spectrum_8"]["n_triangles"] = [int(x) for x in S["n_triangles"]]
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_isovalues_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
