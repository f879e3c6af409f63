#!/usr/bin/env python3
"""per-call times of the regions calls (csrc/cx_regions.hip) on the bench field (512^3, the bench's generator) in one warm process:
  records_shape / records_fp32   cx_grid_regions3d of split_touching's labels ({f >= median}, h = 2): without values, and with the
                                 float32 distance field as values;
  records_noise                  the same of label()'s labels of uniform noise at density 0.5, connectivity 1 (millions of regions; a K
                                 above CX_REGIONS_MAX_LABEL is recorded as the refusal it is and not timed);
  groups_max                     records_fp32 and records_noise at other settings of CXR_GROUPS_MAX (the debug knob CX_REGIONS_GROUPS),
                                 the settings alternating inside every repeat;
  surface_crop / surface_whole   select + bind + march + post-pass of the largest region: cropped to its box with pad 1, and the same
                                 label selected over the whole volume;
  contacts, relabel              cx_grid_regions3d_contacts, and cx_grid_regions3d_map through the sequential table into a second buffer.
Beside each: the traffic floor, one read of the call's inputs (and one write of its output) at the rate cx_measure_read_bandwidth
reports here, and the multiple of it.  As context only, scipy.ndimage.find_objects, sum and maximum_position of the split labels on this
host in seconds (argument 3 = 0 leaves them out: they are then NOT MEASURED).
3 warm + `reps` timed calls, each between two HIP events on the context's stream.  No hardware counter is read.
Prints one JSON line and writes it to profiles/bench_regions_<size>.json."""
import json, os, statistics, sys, time
os.environ["CX_DEBUG"] = "1"      # (before the library loads: the knob CX_REGIONS_GROUPS is honoured)
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch
from contourist_amd import _ffi, synthetic, volume
size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
with_scipy = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
dev = torch.device("cuda", 0)
F = synthetic.smooth_noise_torch((size,) * 3, 1235, 1400, dev)
n = F.numel()
shape = tuple(int(x) for x in F.shape)
ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
median = float(F.view(-1).kthvalue(n // 2 + 1).values)
out = {"size": size, "reps": reps, "device": torch.cuda.get_device_name(0), "samples": n, "median": median, "h": 2.0,
       "hardware_counters_read": False, "groups_max_default": 8}
GBps = ctx.measure_read_bandwidth(F.data_ptr(), n * 4, 5)
out["read_GBps"] = round(GBps, 1)


def once(call):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms, bytes_moved):
    floor_ms = bytes_moved / (GBps * 1e9) * 1e3
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "traffic_floor_ms": round(floor_ms, 4),
            "over_traffic_floor": round(med / floor_ms, 2)}


def timed(name, call, bytes_moved, **extra):
    ms = [once(call) for _ in range(3 + reps)][3:]
    out[name] = dict(summary(ms, bytes_moved), **extra)
    print(name, out[name]["median_ms"], "ms", file=sys.stderr, flush=True)
    write()


def write():
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bench_regions_%d.json" % size), "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


labels = volume.split_touching(F, median, 2.0).contiguous()
D = torch.empty(shape, dtype=torch.float32, device=dev)
ctx.distance_grid(median, "above", "float32", samples=(F.data_ptr(), F.dtype, shape), out=D.data_ptr())
torch.cuda.synchronize()
L, V = (labels.data_ptr(), shape), (D.data_ptr(), "float32", shape)
records = ctx.regions_grid(L, V)
present = records["voxels"] > 0
out["split_labels"] = {"k": len(records), "present": int(present.sum()), "labelled_samples": int(records["voxels"].sum()),
                       "largest_voxels": int(records["voxels"].max())}
# (two passes over the labels: the largest label, then the measures; the records come back over the host link)
timed("records_shape", lambda: ctx.regions_grid(L), 2 * n * 4)
timed("records_fp32", lambda: ctx.regions_grid(L, V), 2 * n * 4 + n * 4)

noise = (torch.rand(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) < 0.5).to(torch.uint8).contiguous()
noise_labels = torch.empty(shape, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
k_noise, _ = ctx.label_grid(0.5, "high", 1, samples=(noise.data_ptr(), "uint8", shape), out=noise_labels.data_ptr())
N = (noise_labels.data_ptr(), shape)
if k_noise > _ffi.CX_REGIONS_MAX_LABEL:
    try:
        ctx.regions_grid(N)
        out["records_noise"] = {"k": int(k_noise), "refused": False}
    except _ffi.CxError as e:
        out["records_noise"] = {"k": int(k_noise), "refused": True, "code": e.code, "timed": False}
else:
    timed("records_noise", lambda: ctx.regions_grid(N), 2 * n * 4, k=int(k_noise), host_copy_bytes=int(k_noise) * 128)

# CXR_GROUPS_MAX: the settings alternate inside every repeat, so that a drift of the machine touches all of them alike
settings = (1, 2, 4, 8, 16, 64)
cases = {"records_fp32": lambda: ctx.regions_grid(L, V)}
if "median_ms" in out.get("records_noise", {}):
    cases["records_noise"] = lambda: ctx.regions_grid(N)
compare = {name: {g: [] for g in settings} for name in cases}
for r in range(2 + reps):
    for g in settings:
        os.environ["CX_REGIONS_GROUPS"] = str(g)
        for name, call in cases.items():
            ms = once(call)
            if r >= 2:
                compare[name][g].append(ms)
del os.environ["CX_REGIONS_GROUPS"]
out["groups_max"] = {name: {str(g): {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
                            for g, ms in per.items()} for name, per in compare.items()}
write()

# one surface: the largest region, from its box and from the whole volume
c = int(np.argmax(records["voxels"])) + 1
flags = np.zeros(c + 1, dtype=np.uint8)
flags[c] = 1
box = (records["lo"][c - 1], records["hi"][c - 1])
last = {}


def surface(the_box, pad):
    _, mshape, origin, _ = ctx.regions_select(L, flags, the_box, pad)
    ctx.bind_region_mask()
    ctx.set_origin(*origin)
    counts = ctx.extract3d(0.5)
    last["post"] = ctx.postprocess3d()
    last["mask_samples"] = int(np.prod(mshape))
    ctx.set_origin(0, 0, 0)


ext = [int(h) - int(l) + 3 for l, h in zip(*box)]
timed("surface_crop", lambda: surface(box, 1), int(np.prod(ext)) * 5, label=c, box_lo=[int(x) for x in box[0]], box_hi=[int(x) for x in box[1]])
out["surface_crop"].update(mask_samples=last["mask_samples"], n_vertices=last["post"]["n_vertices"], n_triangles=last["post"]["n_triangles"])
timed("surface_whole", lambda: surface(None, 0), n * 5, label=c)
out["surface_whole"].update(mask_samples=last["mask_samples"], n_vertices=last["post"]["n_vertices"], n_triangles=last["post"]["n_triangles"])
out["surface_whole_over_crop"] = round(out["surface_whole"]["median_ms"] / out["surface_crop"]["median_ms"], 2)

pairs = ctx.regions_contacts(L)
timed("contacts", lambda: ctx.regions_contacts(L), n * 4, pairs=len(pairs), faces=int(pairs["faces"].sum()))
forward = np.zeros(len(records) + 1, dtype=np.int32)
forward[1:][present] = np.arange(1, int(present.sum()) + 1)
mapped = torch.empty(shape, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
timed("relabel", lambda: ctx.regions_map(L, forward, out=mapped.data_ptr()), 2 * n * 4)
out["device_bytes_at_end"] = _ffi.device_bytes(ctx.handle)[0]
out["scipy"] = "not measured"
write()
if with_scipy:
    import scipy.ndimage as ndi
    host_labels, host_values = labels.cpu().numpy(), D.cpu().numpy()
    index = np.arange(1, len(records) + 1)
    took = {}
    for name, call in (("find_objects", lambda: ndi.find_objects(host_labels)), ("sum", lambda: ndi.sum(host_values, host_labels, index)),
                       ("maximum_position", lambda: ndi.maximum_position(host_values, host_labels, index))):
        t0 = time.time()
        call()
        took[name + "_s"] = round(time.time() - t0, 2)
        out["scipy"] = dict(took)
        write()
ctx.close()
print(json.dumps(out))
