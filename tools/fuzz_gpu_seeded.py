#!/usr/bin/env python3
"""Randomised parity of the seeded selections (cx_select_seeded3d_ex, cx_select_seeded4d_ex: the two-step unions, the keep kernels, both
seed kernels) on the GPU: random multi-component fields of noisy spheres (several thousand surface voxels: many blocks of records, pairs
across blocks), random far-apart end point pairs that the device has to bisect, random in_range boxes (now and then empty or beyond the
array), now and then CX_SEED_ALL_IN_RANGE and the one-thread-per-pair seed kernel -- kept simplices, counts, vertex mask and groups_kept
against oracle/seeds.py.  Fields, cases and the comparison are those of the test suite (tests/seeded_cases.py).
python tools/fuzz_gpu_seeded.py [seconds] [seed] [3|4: dimension, default both in turn]"""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import seeded_cases as sc
from oracle import seeds
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
rng = np.random.RandomState(int(sys.argv[2]) if len(sys.argv) > 2 else 17)
dims = (int(sys.argv[3]),) if len(sys.argv) > 3 else (3, 4)
t0 = time.time(); last_note = t0; ncase = 0; nbad = 0; nkept = 0; nfield = 0
while time.time() - t0 < budget:
    if time.time() - last_note > 60.0:
        last_note = time.time()
        print("... %d cases, %d mismatches, %.0f s" % (ncase, nbad, time.time() - t0), flush=True)
    dim = dims[nfield % len(dims)]
    A, v = sc.random_field(rng, dim)
    sizes = [n for n, _ in seeds.groups(A, v, ())]
    if np.any(A == v) or len(sizes) < 2 or not np.any(A < v):       # (no sample equal to the isovalue; more than one component)
        continue
    nfield += 1
    M = sc.OracleMesh(A, v)
    D = sc.DeviceMesh(A, v)
    try:
        for trial in range(4):
            c = sc.random_case(rng, A, v)
            r = sc.run_case(D, M, c)
            ncase += 1; nkept += int(r["want"].sum())
            if r["mismatches"]:
                nbad += 1
                print("MISMATCH shape", A.shape, "components", sizes, "case", c, r["got"], r["mismatches"], flush=True)
    finally:
        D.close()
print("fuzz seeded selection: %d cases on %d fields, %d simplices kept, %d mismatches, %.0f s" % (ncase, nfield, nkept, nbad, time.time() - t0))
sys.exit(1 if nbad else 0)
