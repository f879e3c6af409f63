"""bench.py --dump-outputs: the files name the Level-0 mesh whatever order the device emitted it in, stay within their
size bound, and hold float arrays only.  CPU part: dump_outputs on a stand-in context; GPU part: two runs of the bench
with the same arguments dump the same files, and --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeContext(object):
    "what dump_outputs reads of a context: counts() and download_level0()"

    def __init__(self, xyz, keys, tris):
        self.xyz, self.keys, self.tris = xyz, keys, tris

    def counts(self):
        return {"n_cells": 7, "n_vertices": len(self.keys), "n_triangles": len(self.tris), "n_border_voxels": 5}

    def download_level0(self, counts):
        assert counts == self.counts()
        return self.xyz.copy(), self.keys.copy(), self.tris.copy()


def random_mesh(rng, nv, nt):
    keys = rng.choice(1 << 31, size=nv, replace=False).astype(np.uint32)
    xyz = rng.standard_normal((nv, 3)).astype(np.float32)
    tris = np.stack([rng.choice(nv, size=3, replace=False) for _ in range(nt)]).astype(np.int32)
    return xyz, keys, tris


def reordered(xyz, keys, tris, rng):
    "the same mesh emitted in another order: vertices permuted, triangles permuted and each rotated (winding kept)"
    perm = rng.permutation(len(keys))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    t = inv[tris][rng.permutation(len(tris))]
    rot = rng.randint(0, 3, size=len(t))
    t = np.take_along_axis(t, (rot[:, None] + np.arange(3)[None, :]) % 3, axis=1)
    return xyz[perm], keys[perm], t.astype(np.int32)


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("small_rows", [False, True])
def test_dump_is_independent_of_emission_order(tmp_path, monkeypatch, small_rows):
    if small_rows:
        monkeypatch.setattr(bench, "DUMP_ROWS", 500)        # the mesh is larger than the sample: hashed selection and the cap
    rng = np.random.RandomState(3)
    xyz, keys, tris = random_mesh(rng, 3000, 6000)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    shapes = bench.dump_outputs(FakeContext(xyz, keys, tris), a)
    bench.dump_outputs(FakeContext(*reordered(xyz, keys, tris, rng)), b)
    A, B = load(a), load(b)
    assert sorted(A) == sorted(shapes) == ["counts", "triangle_edge_ids", "vertex_edge_ids", "vertex_xyz"]
    for name in A:
        assert A[name].dtype in (np.float32, np.float64), (name, A[name].dtype)
        assert list(A[name].shape) == shapes[name]
        assert np.array_equal(A[name], B[name]), name
    assert list(A["counts"]) == [7, 3000, 6000, 5]
    cap = bench.DUMP_ROWS
    nv, nt = len(A["vertex_edge_ids"]), len(A["triangle_edge_ids"])
    if small_rows:
        assert 0.8 * cap < nv <= cap and 0.8 * cap < nt <= cap
    else:
        assert nv == 3000 and nt == 6000
    # the rows are the mesh's own: vertex ids with their coordinates, triangles as corner ids starting at the smallest, winding kept
    where = {int(k): i for i, k in enumerate(keys)}
    ids = A["vertex_edge_ids"].astype(np.int64)
    assert np.all(np.diff(ids) > 0)
    assert np.array_equal(A["vertex_xyz"], xyz[[where[k] for k in ids]])
    own = {tuple(int(x) for x in np.roll(keys[t], -int(np.argmin(keys[t])))) for t in tris}
    T = A["triangle_edge_ids"].astype(np.int64)
    assert all(tuple(int(x) for x in row) in own for row in T)
    assert np.all(T[:, 0] < T[:, 1]) and np.all(T[:, 0] < T[:, 2])


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and b"--steps must be at least 1" in p.stderr


def run_bench(*argv):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(lines[0])


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs(tmp_path):
    common = ["--size", "128", "--passes", "40", "--rotate", "4", "--steps", "3", "--warmup", "1",
              "--no-cpu-baseline", "--no-api", "--no-config4", "--levels", "0", "--no-single-stream"]
    one = run_bench("--dump-outputs", str(tmp_path / "a"), *common)
    two = run_bench("--dump-outputs", str(tmp_path / "b"), *common)
    assert one["steps"] == two["steps"] == 3 and one["ms_per_step"] > 0 and two["ms_per_step"] > 0
    A, B = load(str(tmp_path / "a")), load(str(tmp_path / "b"))
    assert sorted(A) == ["counts", "triangle_edge_ids", "vertex_edge_ids", "vertex_xyz"]
    assert sum(a.nbytes for a in A.values()) <= 64 << 20
    for name in A:
        assert np.array_equal(A[name], B[name]), name
    assert A["counts"][1] == one["config"]["vertices_rank0"] and A["counts"][2] == one["config"]["triangles_rank0"]
    for name, n in (("vertex_edge_ids", A["counts"][1]), ("triangle_edge_ids", A["counts"][2])):
        rows = len(A[name])
        assert rows == n if n <= bench.DUMP_ROWS else 0.8 * bench.DUMP_ROWS < rows <= bench.DUMP_ROWS, (name, rows, n)
