#!/usr/bin/env python3
"""Typed 3-D grids against fp32 on the same values: the 512^3 bench field (synthetic.smooth_noise_host, seed 1235, what bench.py
extracts) quantised to int16 and uint8, and the same values as fp32, in one process, measured alternately:
  - Level 0 ms: one extraction after the other, and two in flight (two contexts on two streams);
  - the host -> device upload from pageable memory (cx_grid_upload_typed against cx_grid_upload);
  - the TriangulatedIsosurfaces(..., array, ...).get_points_and_triangles() API time (bind, Level 0, Level 1, download).
One JSON line per type.  --profile: only a few extractions per type (for a rocprofv3 --kernel-trace --stats run of its own)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from contourist_amd import _ffi, synthetic, tetrahedral


def quantise(y, name):
    "(typed array, its fp32 copy, the isovalue: halfway between the two samples around the fp32 field's 0)"
    if name == "int16":
        s = 30000.0 / float(np.abs(y).max())
        q = np.rint(y * s).astype(np.int16)
        return q, q.astype(np.float32), 0.5
    lo, hi = float(y.min()), float(y.max())
    q = np.rint((y - lo) / (hi - lo) * 254.0).astype(np.uint8)
    return q, q.astype(np.float32), float(np.floor(-lo / (hi - lo) * 254.0)) + 0.5


def sync():
    torch.cuda.synchronize()


def one_after_the_other(ctxs, value, reps):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctxs[0].extract3d(value)
    sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def two_in_flight(ctxs, value, reps):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctxs[0].extract3d_async(value)
        ctxs[1].extract3d_async(value)
        ctxs[0].counts()
        ctxs[1].counts()
    sync()
    return (time.perf_counter() - t0) * 1e3 / (2 * reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--passes", type=int, default=1400)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--types", default="int16,uint8")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    n = args.size
    y = synthetic.smooth_noise_host((n, n, n), 1235, args.passes)
    for name in args.types.split(","):
        q, f32, value = quantise(y, name)
        streams = [torch.cuda.Stream() for _ in range(2)]
        typed = [_ffi.Context(0, stream=s.cuda_stream) for s in streams]
        plain = [_ffi.Context(0, stream=s.cuda_stream) for s in streams]
        for c in typed:
            c.upload_grid_native(q)
        for c in plain:
            c.upload_grid(f32)
        assert typed[0].grid_info() == dict(dtype=name, device_bytes=q.nbytes)
        a, b = typed[0].extract3d(value), plain[0].extract3d(value)
        assert a == b, (a, b)
        if args.profile:
            for _ in range(5):
                typed[0].extract3d(value)
                plain[0].extract3d(value)
            sync()
            print(json.dumps(dict(dtype=name, profile_run=True, counts=a)))
            continue
        res = {k: ([], []) for k in ("level0_ms", "level0_two_in_flight_ms", "upload_ms", "api_ms")}
        for _ in range(args.rounds):
            for side, ctxs, arr in ((0, typed, q), (1, plain, f32)):     # alternating: typed, fp32, typed, ...
                res["level0_ms"][side].append(one_after_the_other(ctxs, value, args.reps))
                res["level0_two_in_flight_ms"][side].append(two_in_flight(ctxs, value, args.reps))
                sync()
                t0 = time.perf_counter()
                if side == 0:
                    ctxs[0].upload_grid_native(arr)
                else:
                    ctxs[0].upload_grid(arr)
                sync()
                res["upload_ms"][side].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                S = tetrahedral.TriangulatedIsosurfaces([0.0] * 3, [1.0] * 3, [1.0 / n] * 3, arr, value, [])
                p, t = S.get_points_and_triangles()
                res["api_ms"][side].append((time.perf_counter() - t0) * 1e3)
        out = dict(dtype=name, size=n, value=value, n_triangles=a["n_triangles"], device_bytes=dict(typed=q.nbytes, fp32=f32.nbytes))
        for k, (tv, fv) in res.items():
            out[k] = dict(typed=round(float(np.median(tv)), 4), fp32=round(float(np.median(fv)), 4))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
