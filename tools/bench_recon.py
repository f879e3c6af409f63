#!/usr/bin/env python3
"""per-call times of cx_grid_reconstruct3d on the bench field (512^3, the bench's generator), the fp32 field and a uint8 copy of it (256
steps between its minimum and maximum), connectivity 1, in one warm process:
  h_maxima      CX_RECON_MARKER_SHIFT with h = a tenth of the value range (uint8: 26);
  regional_maxima  CX_RECON_MARKER_STEP, CHANGED, of the float32 distance() field of the field thresholded at its median;
  fill_holes_grey  CX_RECON_MARKER_RIM, all faces, erosion;
  propagate     a uint8 marker array with one seed, through the mask {f >= median}.
Beside each time: the rounds and tile visits of the last call, and the multiple of the traffic floor: one read of every input plus one
write of the result at the rate cx_measure_read_bandwidth reports here.
Two baselines, measured in the same process:
  the naive device loop: one round = cx_grid_rank3d maximum over 3^3 (connectivity 3's structure; the separable kernel) plus
  torch.minimum with the mask, `naive_rounds` rounds timed, reported per round.  It advances one sample per round, this call's rounds one
  tile boundary at least, so (rounds - 1) naive rounds is a LOWER bound of what the naive loop needs: the extrapolation uses that;
  on the host, scipy.ndimage.binary_propagation for the binary case, with equality asserted (argument 3 = 0 leaves it out).
3 warm + `reps` timed calls, each between two HIP events on the context's stream; the result goes into the context's own buffer.
Prints one JSON line and writes it to profiles/bench_recon_<size>.json."""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from contourist_amd import _ffi, synthetic
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
with_scipy = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
naive_rounds = 8
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


out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n, "connectivity": 1, "median": median}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)


def case(name, T, marker, out_bytes_per_sample=None, **kw):
    samples = (T.data_ptr(), T.dtype, shape)
    last = {}

    def call():
        last["stats"] = ctx.reconstruct_grid(marker, samples=samples, **kw)[0]
    r = timed(call)
    esize = T.element_size()
    inputs = esize * (1 if isinstance(marker, str) else 2)
    floor_ms = n * (inputs + (esize if out_bytes_per_sample is None else out_bytes_per_sample)) / (GBps * 1e9) * 1e3
    r.update(last["stats"])
    r.update(traffic_floor_ms=round(floor_ms, 4), over_traffic_floor=round(r["median_ms"] / floor_ms, 2),
             tiles=int(np.prod([-(-s // t) for s, t in zip(shape, (8, 8, 64))])))
    out[name] = r
    print(name, r["median_ms"], "ms", r["rounds"], "rounds", file=sys.stderr, flush=True)
    return r


def naive(name, T, start, rounds_needed):
    "the naive loop from the marker `start` under the mask T: `naive_rounds` rounds of maximum 3^3 and torch.minimum"
    cur = start.clone()
    nxt = torch.empty_like(cur)

    def call():
        nonlocal cur, nxt
        for _ in range(naive_rounds):
            ctx.rank_grid(3, 26, samples=(cur.data_ptr(), cur.dtype, shape), out=nxt.data_ptr())
            torch.minimum(nxt, T, out=cur)
    r = timed(call, 3)
    per_round = r["median_ms"] / naive_rounds
    out[name].update(naive_ms_per_round=round(per_round, 4), naive_rounds_lower_bound=max(1, rounds_needed - 1),
                     naive_extrapolated_ms_at_least=round(per_round * max(1, rounds_needed - 1), 2))


h8 = 26
r = case("h_maxima_fp32", F, "shift", h=0.1 * (hi - lo))
naive("h_maxima_fp32", F, F - 0.1 * (hi - lo), r["rounds"])
r = case("h_maxima_uint8", U, "shift", h=h8)
naive("h_maxima_uint8", U, (U.to(torch.int16) - h8).clamp(0, 255).to(torch.uint8), r["rounds"])
D = torch.empty(shape, dtype=torch.float32, device=dev)
ctx.distance_grid(median, "below", "float32", samples=(F.data_ptr(), F.dtype, shape), out=D.data_ptr())
case("regional_maxima_of_distance", D, "step", out_bytes_per_sample=1, out_kind="changed")
case("fill_holes_grey_fp32", F, "rim", method="erosion")
case("fill_holes_grey_uint8", U, "rim", method="erosion")
M = (F >= median).to(torch.uint8).contiguous()
seed = torch.zeros_like(M)
seed.view(-1)[int(torch.argmax(F))] = 1
torch.cuda.synchronize()
r = case("propagate_uint8", M, (seed.data_ptr(), seed.dtype, shape))
naive("propagate_uint8", M, seed, r["rounds"])
if with_scipy:
    import scipy.ndimage as ndi
    mask_h, seed_h = M.cpu().numpy() != 0, seed.cpu().numpy() != 0
    t0 = time.time()
    want = ndi.binary_propagation(seed_h, mask=mask_h)
    out["propagate_uint8"]["scipy_binary_propagation_s"] = round(time.time() - t0, 2)
    got = ctx.reconstruct_grid((seed.data_ptr(), seed.dtype, shape), samples=(M.data_ptr(), M.dtype, shape), download=True)[1]
    assert np.array_equal(got != 0, want), "the device propagation differs from scipy.ndimage.binary_propagation"
    out["propagate_uint8"]["equals_scipy"] = True
    out["propagate_uint8"]["scipy_over_device"] = round(out["propagate_uint8"]["scipy_binary_propagation_s"] * 1e3 / out["propagate_uint8"]["median_ms"], 1)
    out["propagate_uint8"]["reached"] = int(want.sum())
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles"), exist_ok=True)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "bench_recon_%d.json" % size), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
